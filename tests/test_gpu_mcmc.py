"""GPU tests of 3DGS-MCMC relocation, growth and noise (include/splat.h, "MCMC relocation"; splat_renderer_amd.fit) against
the restatement of tests/mcmc_ref.py, in the manner and with the sentinel-tail buffers of tests/test_gpu_density.py.

Bounds (none taken from the code under test):
  sample   targets, sources, counts and the host words EXACT.  The one place two correct implementations may differ is
           floor(2^24 sigmoid(logit)) between two binary64 exp()s, which can happen only within ~1e-9 of an integer: the tests
           assert on the REFERENCE that every input's 2^24 o is at least 1e-6 from an integer (seeds chosen on the CPU so that it
           holds), and drop nothing.  Among the million logits of a cloud past 256 block sums two or three do lie that close:
           MR.off_integers moves those to the next float32, and the same assertion then holds there too.
  apply    copies bit for bit, moments exact zeros or kept bits, new logits and log-scales within 1 binary32 ulp (taken at
           max(|x|, 2^-10)) of the float64 restatement: the binary64 error of the sum, below 1e-12, can only flip the final
           rounding.
  noise    |delta - float64| <= 1e-4 sigma_max^2 |xi|_2 g scale + 1 ulp(|mu|): ten times the dominant term, a binary32
           sigmoid's ~1e-7 relative error in o times the gate's 100, beside some thirty binary32 operations; the ulp is the final
           add's rounding.
Every test prints the figures it asserts on.
"""
import ctypes as C
import time

import numpy as np
import pytest
import torch

import splat_renderer_amd as sr
from splat_renderer_amd import _lib
from splat_renderer_amd import autograd as AG
from tests import mcmc_ref as MR
from tests import test_gpu_density as TD

pytestmark = pytest.mark.gpu

_dev, _ptr, _host, _lib_ctx, ulp32 = TD._dev, TD._ptr, TD._host, TD._lib_ctx, TD.ulp32
MIN_OPACITY = 0.005
SEED = 0xC0FFEE_0000_0002
bits = lambda a: np.ascontiguousarray(a).view(np.uint32)  # noqa: E731


def assert_away_from_integers(logits, label):
    x = MR.scaled_opacity(logits)[np.isfinite(logits)]  # (an infinite logit's exp is exact: o is 0 or 1 in any implementation)
    d = float(np.abs(x - np.round(x)).min()) if x.size else 1.0
    assert d >= 1e-6, f"{label}: an input's 2^24 o is {d:.3g} from an integer"
    return d


def sample_gpu(logits, mode, n_draws, seed, min_opacity=MIN_OPACITY):
    """splat_mcmc_sample on the device: (targets, sources, counts, words), targets and sources cut to the draws made; the input,
    the words past the draws and the sentinel tails are checked to be untouched."""
    lib, ctx = _lib_ctx()
    n = logits.shape[0]
    room = max(n if mode == MR.RELOCATE else n_draws, 1)
    L = _dev(logits)
    T, S = _dev(np.full(room, 0xDEADBEEF, np.uint32)), _dev(np.full(room, 0xDEADBEEF, np.uint32))
    Cn = _dev(np.full(max(n, 1), 0xDEADBEEF, np.uint32))
    nbytes = int(lib.splat_mcmc_sample_workspace_bytes(n))
    ws = torch.empty(max(nbytes // 4, 4), device="cuda", dtype=torch.int32)
    words = (C.c_uint32 * 3)(9, 9, 9)
    rc = lib.splat_mcmc_sample(ctx, _ptr(L), n, mode, n_draws, min_opacity, seed, ws.data_ptr(), nbytes, _ptr(T), _ptr(S), _ptr(Cn), words)
    assert rc == 0, lib.splat_last_error(ctx)
    torch.cuda.synchronize()
    assert np.array_equal(_host(*L, np.uint32, logits.shape), bits(logits)), "the logits were written"
    draws = int(words[2])
    t, s = _host(*T, np.uint32, (room,)), _host(*S, np.uint32, (room,))
    assert (t[draws:] == 0xDEADBEEF).all() and (s[draws:] == 0xDEADBEEF).all(), "words past the draws were written"
    return t[:draws], s[:draws], _host(*Cn, np.uint32, (max(n, 1),))[:n], tuple(int(x) for x in words)


def check_sample(logits, label, seed=SEED, min_opacity=MIN_OPACITY, add=None, modes=(MR.RELOCATE, MR.ADD), known=None):
    """Both modes (or `modes`) against MR.sample; known: {mode: MR.sample's result} where the caller has formed it already."""
    d = assert_away_from_integers(logits, label)
    n = logits.shape[0]
    out = {}
    for mode, k in ((MR.RELOCATE, 0), (MR.ADD, n // 20 + 3 if add is None else add)):
        if mode not in modes:
            continue
        want = known[mode] if known and mode in known else MR.sample(logits, mode, k, seed, min_opacity)
        got = sample_gpu(logits, mode, k, seed, min_opacity)
        name = "relocate" if mode == MR.RELOCATE else "add"
        print(f"{label} {name}: (dead, alive, draws) {got[3]}, reference {want[3]}; {int((got[2] > 0).sum())} sources; "
              f"min |2^24 o - integer| {d:.3g}")
        assert got[3] == want[3], f"{label} {name}: host words {got[3]} != {want[3]}"
        for a, b, what in zip(got[:3], want[:3], ("targets", "sources", "counts")):
            assert np.array_equal(a, b), f"{label} {name}: {what} differ"
        out[name] = got
    return out


normal_logits = MR.normal_logits


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257, 4097, 70001])
def test_sample_is_the_restatement(device, n):
    logits = normal_logits(n, 100 + n)
    if n == 1:
        logits[0] = 1.25  # (alive: its draws are all itself)
    got = check_sample(logits, f"n={n}")
    if n >= 4097:
        assert got["relocate"][3][0] >= 0.02 * n and got["add"][3][2] == n // 20 + 3


def test_sample_needs_64_bit_sums(device):
    """70 001 splats near o = 0.9 sum to ~1e12, and 70 001 weights of 2^24 - 1 to 1.17e12: a 32-bit sum fails both."""
    n = 70001
    logits = np.random.default_rng(7).normal(2.2, 0.1, n).astype(np.float32)
    _, _, w = MR.weights(logits, MIN_OPACITY)
    assert int(w.sum()) > 2 ** 39
    got = check_sample(logits, "o ~ 0.9", add=5000)
    assert got["relocate"][3] == (0, n, 0)
    full = np.full(n, 17.0, np.float32)
    q, _, _ = MR.weights(full, MIN_OPACITY)
    assert (q == 2 ** 24 - 1).all()
    check_sample(full, "weights 2^24 - 1", add=5000)


@pytest.mark.parametrize("name", MR.FAR_CASES)
def test_sample_past_256_block_sums(device, name):
    """k_scan64_sums scans the block sums (one per 2048 weights) 256 at a time and carries a 64-bit total from trip to trip: a
    second trip needs n > 524 288.  MR.far_case's clouds: 256 block sums (one trip, full), 257, and 601 (three trips, the last
    partial) of normal logits, whose first trip alone sums past 2^32, so the carry needs its high word; every weight 2^24 - 1;
    and two clouds whose carries are zeros: nobody alive before the third trip, and nobody alive after the first block sum (the
    first trip's total must still arrive unchanged in the last).  MR.far_case_regime asserts all that, and that at least 1000 of
    the 5000 added draws have a source past the first trip, from the restatement before the device is asked (the draws from
    n = 1 229 577 on: at 524 289 one splat lies past the first trip).  Then targets, sources, counts and the host words are
    MR.sample's, in both modes; the two clouds with more than a million dead splats in the add mode only (their relocation
    would be a million draws of Python integers, through the same scan)."""
    logits, alive = MR.far_case(name)
    n = logits.shape[0]
    want = MR.sample(logits, MR.ADD, 5000, SEED, MIN_OPACITY)
    first, total, past = MR.far_case_regime(name, logits, alive, want[1], MIN_OPACITY)
    print(f"{name}: n = {n}, {-(-n // MR.SCAN_TILE)} block sums; weight up to the end of the first trip {first} = 2^{np.log2(max(first, 1)):.1f}, "
          f"total {total}; {past} of 5000 added draws have a source past the first trip")
    modes = (MR.ADD,) if name.startswith("alive") else (MR.RELOCATE, MR.ADD)
    got = check_sample(logits, name, add=5000, modes=modes, known={MR.ADD: want})
    s = got["add"][1]
    assert got["add"][3][2] == 5000 and ((s >= alive[0]) & (s < alive[1])).all()
    if name == "saturated":
        assert got["relocate"][3] == (0, n, 0)


def boundary_logits(min_opacity):
    """The two neighbouring binary32 logits whose q lie on either side of q_min: (last dead, first alive)."""
    lo = np.float32(np.log(min_opacity) - np.log1p(-min_opacity) - 1e-3)
    while True:
        hi = np.nextafter(lo, np.float32(np.inf))
        if not MR.weights(np.array([hi]), min_opacity)[1][0]:
            return lo, hi
        lo = hi


def test_sample_special_clouds(device):
    rng = np.random.default_rng(11)
    alive = rng.normal(1.0, 1.0, 300).astype(np.float32)
    got = check_sample(alive, "nobody dead")
    assert got["relocate"][3] == (0, 300, 0) and not got["relocate"][2].any()
    dead = rng.normal(-9.0, 0.5, 300).astype(np.float32)
    got = check_sample(dead, "everybody dead")
    assert got["relocate"][3] == (300, 0, 0) and got["add"][3] == (300, 0, 0) and not got["add"][2].any()
    one = np.full(101, -8.0, np.float32)
    one[37] = 0.7
    got = check_sample(one, "one alive, 100 dead")
    assert got["relocate"][3] == (100, 1, 100) and (got["relocate"][1] == 37).all() and got["relocate"][2][37] == 100
    odd = normal_logits(200, 12)
    odd[[3, 50, 199]] = np.nan
    odd[[4, 51]] = -np.inf
    odd[[5, 52]] = np.inf
    got = check_sample(odd, "NaN and infinite logits")
    assert set([3, 50, 199, 4, 51]) <= set(got["relocate"][0].tolist()) and not got["relocate"][2][[3, 50, 199, 4, 51]].any()
    for mo in (MIN_OPACITY, 0.3):
        lo, hi = boundary_logits(mo)
        edge = normal_logits(130, 13)
        edge[[0, 64, 129]] = lo
        edge[[1, 65, 128]] = hi
        got = check_sample(edge, f"logits at the q_min boundary of {mo}", min_opacity=mo)
        t = set(got["relocate"][0].tolist())
        assert {0, 64, 129} <= t and not ({1, 65, 128} & t)


def test_sample_is_reproducible(device):
    logits = normal_logits(4097, 100 + 4097)
    a = sample_gpu(logits, MR.RELOCATE, 0, SEED)
    b = sample_gpu(logits, MR.RELOCATE, 0, SEED)
    c = sample_gpu(logits, MR.RELOCATE, 0, SEED + 1)
    assert all(np.array_equal(x, y) for x, y in zip(a[:3], b[:3])) and a[3] == b[3]
    assert np.array_equal(a[0], c[0]) and a[3] == c[3]
    differ = float((a[1] != c[1]).mean())
    print(f"another seed: {differ:.3f} of the sources differ")
    assert differ > 0.9


# ---- apply --------------------------------------------------------------------------------------------------------------------

def fit_planes(rows, logits, seed, sh_floats=48):
    rng = np.random.default_rng(seed)
    planes = dict(means=rng.normal(0, 1, (rows, 3)), log_scales=rng.normal(np.log(0.05), 0.5, (rows, 3)), rotations=rng.normal(0, 1, (rows, 4)),
                  opacity_logits=np.resize(logits, rows), sh=rng.normal(0, 0.3, (rows, sh_floats)))
    planes = {k: np.ascontiguousarray(a, np.float32) for k, a in planes.items()}
    m = {k: rng.normal(0, 1, a.shape).astype(np.float32) for k, a in planes.items()}
    v = {k: (rng.normal(0, 1, a.shape) ** 2).astype(np.float32) for k, a in planes.items()}
    return planes, m, v


def apply_gpu(planes, m, v, targets, sources, counts, n, min_opacity):
    lib, ctx = _lib_ctx()
    rows = planes["means"].shape[0]
    P, M, V = ({k: _dev(d[k]) for k in MR.PLANES} for d in (planes, m, v))
    pl = _lib.McmcPlanes()
    for k, name in enumerate(MR.PLANES):
        pl.param[k], pl.m[k], pl.v[k] = _ptr(P[name]), _ptr(M[name]), _ptr(V[name])
    pl.sh_floats = planes["sh"].shape[1]
    T, S, Cn = _dev(np.asarray(targets, np.uint32)), _dev(np.asarray(sources, np.uint32)), _dev(np.asarray(counts, np.uint32))
    rc = lib.splat_mcmc_apply(ctx, _ptr(T), _ptr(S), _ptr(Cn), n, len(targets), rows, min_opacity, C.byref(pl))
    assert rc == 0, lib.splat_last_error(ctx)
    torch.cuda.synchronize()
    for X, a in ((T, targets), (S, sources), (Cn, counts)):
        assert np.array_equal(_host(*X, np.uint32, (len(a),)), np.asarray(a, np.uint32)), "an input of the apply was written"
    return tuple({k: _host(*D[k], np.float32, d[k].shape) for k in MR.PLANES} for D, d in ((P, planes), (M, m), (V, v)))


def check_apply(label, planes, m, v, targets, sources, counts, n, min_opacity):
    """One apply against the restatement; returns the new opacities of the drawn sources (float64)."""
    gp, gm, gv = apply_gpu(planes, m, v, targets, sources, counts, n, min_opacity)
    rp, rm, rv, touched = MR.apply(planes, m, v, targets, sources, counts, min_opacity)
    for k in ("means", "rotations", "sh"):
        assert np.array_equal(bits(gp[k]), bits(rp[k])), f"{label}: {k}: a row differs from its bit-for-bit copy"
    worst = {}
    for k in ("opacity_logits", "log_scales"):
        assert np.array_equal(bits(gp[k][~touched]), bits(planes[k][~touched])), f"{label}: {k}: an untouched row was written"
        ref = rp[k][touched]
        e = np.abs(gp[k][touched].astype(np.float64) - ref) / ulp32(np.maximum(np.abs(ref), 2.0 ** -10))
        worst[k] = float(e.max()) if e.size else 0.0
        assert np.isfinite(gp[k]).all() and worst[k] <= 1.0, f"{label}: {k} is {worst[k]:.3g} ulp from the restatement"
    for k in MR.PLANES:
        for got, ref, before, what in ((gm, rm, m, "m"), (gv, rv, v, "v")):
            assert np.array_equal(bits(got[k]), bits(ref[k])), f"{label}: {what}[{k}] differs"
            assert not bits(got[k][touched]).any(), f"{label}: {what}[{k}] of a moved row or a drawn source is not an exact zero"
            assert np.array_equal(bits(got[k][~touched]), bits(before[k][~touched]))
    s = np.asarray(sources, np.int64)
    t = np.asarray(targets, np.int64)
    for k in ("opacity_logits", "log_scales"):  # a source's new values and its copies' are the same bits
        assert np.array_equal(bits(gp[k][t]), bits(gp[k][s])), f"{label}: {k}: a copy's bits differ from its source's"
    drawn = np.flatnonzero(np.asarray(counts) > 0)
    assert touched.sum() == len(set(t.tolist())) + drawn.size
    print(f"{label}: {len(t)} draws onto {drawn.size} sources (most drawn {int(np.max(counts, initial=0))} times): new logits "
          f"{worst['opacity_logits']:.3g} ulp, log-scales {worst['log_scales']:.3g} ulp from float64")
    return 1.0 / (1.0 + np.exp(-gp["opacity_logits"][drawn].astype(np.float64)))


@pytest.mark.parametrize("sh_floats", [3, 48])
def test_apply_is_the_restatement(device, sh_floats):
    n = 4097
    logits = normal_logits(n, 100 + n)
    # relocate: in place
    targets, sources, counts, words = MR.sample(logits, MR.RELOCATE, 0, SEED, MIN_OPACITY)
    assert words[2] >= 0.02 * n and counts.max() >= 2
    planes, m, v = fit_planes(n, logits, 1, sh_floats)
    check_apply(f"relocate n={n} sh={sh_floats}", planes, m, v, targets, sources, counts, n, MIN_OPACITY)
    # add: planes of n + k rows, the first n the caller's
    k = 205
    targets, sources, counts, words = MR.sample(logits, MR.ADD, k, SEED, MIN_OPACITY)
    assert words[2] == k and np.array_equal(targets, n + np.arange(k))
    planes, m, v = fit_planes(n + k, logits, 2, sh_floats)
    check_apply(f"add n={n} + {k} sh={sh_floats}", planes, m, v, targets, sources, counts, n, MIN_OPACITY)
    # no draws: nothing is written
    gp, gm, gv = apply_gpu(planes, m, v, np.zeros(0, np.uint32), np.zeros(0, np.uint32), np.zeros(n, np.uint32), n, MIN_OPACITY)
    assert all(np.array_equal(bits(gp[x]), bits(planes[x])) and np.array_equal(bits(gm[x]), bits(m[x])) for x in MR.PLANES)


def test_apply_reaches_the_cap_and_both_clamps(device):
    # one alive and 100 dead: every draw the same source, N capped at 51; min_opacity = 0.3 is reached from below
    one = np.full(101, -8.0, np.float32)
    one[37] = np.float32(np.log(0.9 / 0.1))
    targets, sources, counts, words = MR.sample(one, MR.RELOCATE, 0, SEED, 0.3)
    assert words == (100, 1, 100) and counts[37] == 100
    on, _ = MR.relocation(0.9, 51)
    assert on < 0.3
    planes, m, v = fit_planes(101, one, 3)
    o_new = check_apply("one alive, 100 dead, min_opacity 0.3", planes, m, v, targets, sources, counts, 101, 0.3)
    print(f"N = 51 of o = 0.9: o' = {on:.4g}, clamped to {o_new[0]:.6g}")
    assert abs(o_new[0] - 0.3) <= 1e-7
    # the upper end: o = 1 - 1e-7 with N = 2 (o' = 1 - sqrt(1e-7), below the clamp) and a logit of 34 with N = 2, whose
    # o' = 1 - 4e-8 is above 1 - 2^-23 and is clamped to it
    high = np.full(8, -8.0, np.float32)
    high[2] = np.float32(np.log((1 - 1e-7) / 1e-7))
    high[5] = 34.0
    targets, sources, counts = np.array([0, 1], np.uint32), np.array([2, 5], np.uint32), np.zeros(8, np.uint32)
    counts[[2, 5]] = 1
    assert MR.relocation(1.0 / (1.0 + np.exp(-34.0)), 2)[0] > MR.OPACITY_MAX
    planes, m, v = fit_planes(8, high, 4)
    o_new = check_apply("o = 1 - 1e-7 and logit 34, N = 2", planes, m, v, targets, sources, counts, 8, MIN_OPACITY)
    print(f"new opacities: 1 - {1 - o_new[0]:.4g}, 1 - {1 - o_new[1]:.4g}")
    assert abs((1 - o_new[0]) - np.sqrt(1e-7)) <= 1e-3 * np.sqrt(1e-7) and abs((1 - o_new[1]) - 2.0 ** -23) <= 0.05 * 2.0 ** -23


# ---- noise --------------------------------------------------------------------------------------------------------------------

NOISE_SCALE = 5e5 * 1.6e-4


def noise_gpu(planes, step, seed, offset=0, scale=NOISE_SCALE):
    lib, ctx = _lib_ctx()
    n = planes["means"].shape[0]
    D = {k: _dev(planes[k], offset) for k in ("means", "log_scales", "rotations", "opacity_logits")}
    rc = lib.splat_mcmc_noise(ctx, _ptr(D["means"]), _ptr(D["log_scales"]), _ptr(D["rotations"]), _ptr(D["opacity_logits"]), n, scale, step, seed)
    assert rc == 0, lib.splat_last_error(ctx)
    torch.cuda.synchronize()
    for k in ("log_scales", "rotations", "opacity_logits"):
        assert np.array_equal(_host(*D[k], np.uint32, planes[k].shape), bits(planes[k])), f"{k} was written"
    return _host(*D["means"], np.float32, (n, 3))


# (n & 3 = 1, 0, 2, 3 leftover splats after the vector kernel's whole fours; n = 1 takes the scalar kernel, n = 4 is the first vector size)
@pytest.mark.parametrize("n", [1, 4, 6, 7, 8, 65, 4096, 4097, 4098, 4099])
def test_noise_against_float64(device, n):
    logits = normal_logits(n, 200 + n)
    if n == 1:
        logits[0] = -6.0
    planes, _, _ = fit_planes(n, logits, 5)
    step, seed = 17, SEED
    got = noise_gpu(planes, step, seed)
    delta, magnitude, g, o = MR.noise(planes["log_scales"], planes["rotations"], logits, NOISE_SCALE, step, seed)
    mu = planes["means"].astype(np.float64)
    bound = 1e-4 * magnitude[:, None] + ulp32(np.maximum(np.abs(planes["means"]), np.abs(got)))
    e = float((np.abs((got.astype(np.float64) - mu) - delta) / bound).max())
    opaque = o >= 0.5
    moved_opaque = float(np.abs(got.astype(np.float64) - mu)[opaque].max()) if opaque.any() else 0.0
    print(f"noise n={n}: worst |delta - float64| / bound {e:.3g}; {int(opaque.sum())} splats with o >= 0.5 move by at most {moved_opaque:.3g}; "
          f"median |delta| where o < 0.01: {float(np.median(np.abs(delta)[o < 0.01])) if (o < 0.01).any() else 0:.3g}")
    assert np.isfinite(got).all() and e <= 1.0
    assert moved_opaque < 1e-20 * NOISE_SCALE
    # the scalar form (planes 4 bytes past a 16-byte boundary) and a second call: the same bits
    assert np.array_equal(bits(noise_gpu(planes, step, seed, offset=1)), bits(got)), "aligned and misaligned planes differ"
    assert np.array_equal(bits(noise_gpu(planes, step, seed)), bits(got)), "two identical calls differ"
    low = o < 0.01
    if n >= 65:
        assert low.sum() >= 3
        for other in (noise_gpu(planes, step + 1, seed), noise_gpu(planes, step, seed + 1)):
            differ = float((np.abs(other - got).max(axis=1) > 0)[low].mean())
            print(f"another step or seed: {differ:.4f} of the {int(low.sum())} splats with o < 0.01 move differently")
            assert differ >= 0.99


# ---- rejections -----------------------------------------------------------------------------------------------------------------

def test_mcmc_rejections(device):
    lib, ctx = _lib_ctx()
    t = torch.zeros(1 << 16, device="cuda")
    p = t.data_ptr()
    words = (C.c_uint32 * 3)()
    big = 1 << 40
    assert lib.splat_mcmc_sample(ctx, p, 16, 1, 0, 0.005, 0, p + 4096, big, p + 1024, p + 2048, p + 3072, words) == 0
    assert lib.splat_mcmc_sample(ctx, None, 0, 1, 0, 0.005, 0, None, 0, None, None, None, words) == 0 and tuple(words) == (0, 0, 0)  # n = 0
    assert lib.splat_mcmc_sample(ctx, p, 1 << 30, 1, 0, 0.005, 0, p, big, p, p, p, words) == -1
    assert lib.splat_mcmc_sample(ctx, p, 16, 2, 1 << 30, 0.005, 0, p, big, p, p, p, words) == -1
    assert lib.splat_mcmc_sample(ctx, p, 16, 3, 0, 0.005, 0, p, big, p, p, p, words) == -1        # no such mode
    assert lib.splat_mcmc_sample(ctx, None, 16, 1, 0, 0.005, 0, p, big, p, p, p, words) == -1
    assert lib.splat_mcmc_sample(ctx, p + 2, 16, 1, 0, 0.005, 0, p, big, p, p, p, words) == -1    # a misaligned plane
    assert lib.splat_mcmc_sample(ctx, p, 16, 1, 0, 0.005, 0, p + 4, big, p, p, p, words) == -1    # a misaligned workspace
    assert lib.splat_mcmc_sample(ctx, p, 16, 1, 0, 0.005, 0, p, 64, p, p, p, words) == -1         # a small workspace
    assert lib.splat_mcmc_sample(ctx, p, 16, 1, 0, 1.5, 0, p, big, p, p, p, words) == -1
    assert lib.splat_mcmc_sample(ctx, p, 16, 1, 0, 0.005, 0, p, big, p, p, p, None) == -1
    pl = _lib.McmcPlanes()
    for k in range(5):
        pl.param[k], pl.m[k], pl.v[k] = p, p, p
    pl.sh_floats = 48
    assert lib.splat_mcmc_apply(ctx, p, p, p, 16, 0, 16, 0.005, C.byref(pl)) == 0                  # no draws: nothing launched
    assert lib.splat_mcmc_apply(ctx, p, p, p, 16, 4, 8, 0.005, C.byref(pl)) == -1                  # fewer rows than splats
    assert lib.splat_mcmc_apply(ctx, None, p, p, 16, 4, 16, 0.005, C.byref(pl)) == -1
    assert lib.splat_mcmc_apply(ctx, p, p, p, 16, 4, 16, 0.005, None) == -1
    pl.sh_floats = 0
    assert lib.splat_mcmc_apply(ctx, p, p, p, 16, 4, 16, 0.005, C.byref(pl)) == -1
    pl.sh_floats, pl.param[1] = 48, None
    assert lib.splat_mcmc_apply(ctx, p, p, p, 16, 4, 16, 0.005, C.byref(pl)) == -1
    assert lib.splat_mcmc_noise(ctx, None, None, None, None, 0, 1.0, 0, 0) == 0                     # n = 0
    assert lib.splat_mcmc_noise(ctx, p, p, p, None, 16, 1.0, 0, 0) == -1
    assert lib.splat_mcmc_noise(ctx, p + 2, p, p, p, 16, 1.0, 0, 0) == -1
    assert lib.splat_mcmc_noise(ctx, p, p, p, p, 1 << 30, 1.0, 0, 0) == -1
    torch.cuda.synchronize()


# ---- the fit --------------------------------------------------------------------------------------------------------------------

def run_mcmc_fit(u, w, h, target, start, exact_activations=True):
    fit = sr.GaussianFit(start["means"], start["scales"], start["rotations"], start["opacity"], start["sh"], sparse=False,
                         exact_activations=exact_activations)
    counts, events, dead_after = [fit.n], [], None
    for step in range(1, TD.FIT_STEPS + 1):
        rgb, _ = fit.render(u, w, h)
        (AG.photometric_loss(rgb, target) + fit.regularizer()).backward()
        fit.step()
        fit.inject_noise()
        if step % 100 == 0 and step <= 400:
            moved = fit.relocate()
            dead_after = int(MR.weights(fit.opacity_logits.detach().cpu().numpy(), MIN_OPACITY)[1].sum())
            grown = fit.add_new(max_splats=TD.FIT_CAP)
            events.append((moved, grown))
            counts.append(fit.n)
            assert grown["n"] == fit.n and all(getattr(fit, k).shape[0] == fit.n for k in MR.PLANES)
            assert all(x.shape[0] == fit.n for x in (fit.grad_accum, fit.denom, fit.max_radius, fit.visible))
    with torch.no_grad():
        rgb, _ = fit.render(u, w, h)
        loss = float(AG.photometric_loss(rgb, target))
    return fit, loss, rgb, counts, events, dead_after


def test_mcmc_improves_the_fit(device, tmp_path):
    """tests/test_gpu_density.py's scene, 600 steps from 250 splats, three seeds.  A: no density control.  B: 3DGS-MCMC, a dense
    Adam on the loss plus fit.regularizer(), inject_noise() after every step, relocate() then add_new(max_splats=4000) every 100
    steps up to step 400.  Asserted: everything finite; B's count never falls, grows and stays within the cap; after the last
    relocate no splat is dead (by the rule of splat_mcmc_sample); B's final photometric loss (without the regulariser) is not
    above A's; the saved PLY renders to B's last frame within 1e-5; the whole test takes under a minute.  The densify_and_prune
    run's loss is printed beside them for information: no ratio between the two strategies is asserted.

    B is built with exact_activations=True (exp and sigmoid in float64, rounded once, as load_gaussian_ply forms them).  With the
    default float32 activations an ulp of difference in some scales and opacities now and then carries ONE pixel across a splat's
    3-sigma cut, a step of up to 0.011 x opacity: measured on an MI355X over 24 fits of this scene (8 per seed), the round trip of
    a float32-activation B exceeded 1e-5 in 2 of them, in one pixel each (3.9e-4 and 4.2e-3; 3 of 27 in an earlier run of this
    test's own loop), and in 0 of 24 with exact activations, where it was exactly 0."""
    t0 = time.time()
    for seed in (1, 2, 3):
        u, w, h, target, start = TD.fit_scene(seed)
        fit_a, loss_a, _, _, _ = TD.run_fit(u, w, h, target, start, False)
        fit_b, loss_b, rgb_b, counts, events, dead_after = run_mcmc_fit(u, w, h, target, start)
        _, loss_c, _, counts_c, _ = TD.run_fit(u, w, h, target, start, True)
        print(f"seed {seed}: A (250 splats, no density control) loss {loss_a:.5f}; B (MCMC) loss {loss_b:.5f}, counts {counts}, dead after the "
              f"last relocate {dead_after}, events {events}; densify_and_prune loss {loss_c:.5f}, counts {counts_c}")
        for fit in (fit_a, fit_b):
            assert all(torch.isfinite(p).all() for p in fit.parameters())
            assert all(torch.isfinite(x).all() for x in list(fit.m.values()) + list(fit.v.values()))
        assert np.isfinite(loss_a) and np.isfinite(loss_b)
        assert all(b >= a for a, b in zip(counts, counts[1:])) and counts[-1] > counts[0] and max(counts) <= TD.FIT_CAP, counts
        assert dead_after == 0, f"seed {seed}: {dead_after} splats are dead after the last relocate"
        path = str(tmp_path / f"mcmc{seed}.ply")
        fit_b.save_ply(path)
        g = sr.load_gaussian_ply(path)
        assert g["positions"].shape[0] == fit_b.n and g["degree"] == 0
        cloud = sr.GaussianCloud.fromArrays(device, g["positions"], g["scales"], g["rotations"], opacity=g["opacity"], sh=g["sh"])
        r = sr.Renderer(device, None, "rgba8unorm", fit_b.n, footprint="ellipsoid")
        r.render(u, cloud, None, None, w, h, wantFloat=True)
        img = r.readPixelsFloat()[..., :3]
        r.destroy()
        cloud.destroy()
        d = float(np.abs(img - rgb_b.cpu().numpy()).max())
        print(f"seed {seed}: saved PLY renders within {d:.3g} of B's last frame")
        assert d <= 1e-5
        assert loss_b <= loss_a, f"seed {seed}: with MCMC {loss_b:.5f}, without {loss_a:.5f}"
    elapsed = time.time() - t0
    print(f"fit: {elapsed:.1f} s")
    assert elapsed < 60
