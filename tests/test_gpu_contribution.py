"""GPU tests of splat_composite_contribution (include/splat.h, "Contribution of every splat to a frame") through the C ABI: per
splat the hit count, the largest and the summed blend weight of a frame, against the float64 replay of the binary32 composite's
own decisions (tests/contribution_ref.py) and against the kernels that already compute parts of it (the alpha AOV; the colour
column of the composite's backward).

pixel_weight is 0 on the pixels `decisions` marks rim or near (where the kernel's rounding may put a cut or a stop elsewhere), the
device the gradient tests use with their upstream: both sides then evaluate the same function.

weight_max against the float64 reference, largest |got - want| / max(want) measured over the three CASES on an MI355X: 7.92e-08,
2.01e-07 and 1.53e-07 (about three ulps of the largest weight: the hardware exp2 and the binary32 T); the assert is four times
the largest of them, WMAX_TOL, in place of the project's elementwise 2e-3 max(want).
"""
import ctypes as C
import functools

import numpy as np
import pytest

from splat_renderer_amd import _lib
from tests import cameras as CAM
from tests import contribution_ref as CR
from tests import ellipsoid_grad_ref as GR
from tests import ellipsoid_ref as ER
from tests import test_gpu_ellipsoid_grad as TG
from tests import test_gpu_grad_decisions as TD

pytestmark = pytest.mark.gpu

CASES = [  # n, w, h, seed, spread, scale: whole tiles; a ragged bottom row; ragged right and bottom tiles.  Every case walks lists
    # longer than the kernel's 64-entry chunk (474, 329, 798 entries) and has thousands of pixels that stop early
    (500, 64, 64, 3, 0.5, 0.2),
    (3000, 160, 120, 1, 1.0, 0.03),
    (2000, 77, 53, 7, 1.0, 0.05),
]
WMAX_TOL = 4 * 2.01e-7  # x max(want): four times the measured deviation (the module's docstring)
MIN_WEIGHT = 0.01
INVALID = -1
PRIOR = (7, np.float32(1e-30), 12345)  # a non-zero fill of hits, weight_max, weight_sum: untouched splats must keep it


class Scene:
    """One case under one camera: the arrays, the reference's decisions and the rim / near mask."""

    def __init__(self, n, w, h, seed, spread, scale, u=None):
        self.n, self.w, self.h = n, w, h
        pos, scl, rot, self.col = ER.make_cloud(n, seed, spread, scale)
        self.rec, self.counts, self.offsets, self.idx = TG.lists(TG.camera_u(w, h) if u is None else u, pos, scl, rot, w, h)
        self.dec = GR.decisions(self.rec, self.col, self.idx, self.counts, self.offsets, w, h)
        self.bad = self.dec["rim"] | self.dec["near"]
        self.mask = (~self.bad).astype(np.float32)

    @functools.lru_cache(maxsize=None)
    def ref(self, min_weight=0.0, masked=True):
        return CR.contribution(self.dec, self.n, self.w, self.h, self.mask if masked else None, min_weight)


@functools.lru_cache(maxsize=None)
def scene(case, camera=None):
    n, w, h = case[:3]
    u = None if camera is None else CAM.orbit(w, h, azimuth=2.3, elevation=-0.4)
    return Scene(*case, u=u)


class Run:
    """A scene's buffers on the device and calls of the entry point on them."""

    def __init__(self, d, s):
        self.d, self.s = d, s
        self.bufs = [d.createBufferFrom(np.ascontiguousarray(a)) for a in
                     (s.rec, s.col, s.idx if s.idx.size else np.zeros(1, np.uint32), s.counts, s.offsets)]
        self.pw = d.createBuffer(s.w * s.h * 4)
        self.out = [d.createBuffer(max(s.n * 4, 16)), d.createBuffer(max(s.n * 4, 16)), d.createBuffer(max(s.n * 8, 16))]

    def fill(self, hits=0, wmax=0.0, wsum=0):
        n = self.s.n
        self.out[0].write(np.full(n, hits, np.uint32))
        self.out[1].write(np.full(n, wmax, np.float32))
        self.out[2].write(np.full(n, wsum, np.uint64))

    def call(self, mask=None, min_weight=0.0, cfg=None, outs=(True, True, True), offsets=(0, 0, 0), rec_offset=0, pw_offset=0):
        s, b = self.s, self.bufs
        if mask is not None:
            self.pw.write(np.ascontiguousarray(mask, np.float32))
        ptrs = [(o.ptr + off) if on else None for o, on, off in zip(self.out, outs, offsets)]
        return self.d.lib.splat_composite_contribution(self.d.ctx, C.byref(cfg or TG.cfg()), b[1].ptr, 1, b[0].ptr + rec_offset, b[2].ptr, b[3].ptr,
                                                       b[4].ptr, s.w, s.h, (self.pw.ptr + pw_offset) if mask is not None else None, min_weight,
                                                       s.n, *ptrs)

    def read(self):
        n = self.s.n
        return self.out[0].read(np.uint32, n), self.out[1].read(np.float32, n), self.out[2].read(np.uint64, n)

    def destroy(self):
        for b in self.bufs + [self.pw] + self.out:
            b.destroy()


def check_against(ref, hits, wmax, wsum, exact_hits, what=""):
    """The asserts of one result (priors already removed) against a reference dict."""
    if exact_hits:
        assert np.array_equal(hits.astype(np.int64), ref["pairs"]), f"{what}: hits differ from the pair counts"
    else:
        assert (ref["hits_lo"] <= hits).all() and (hits <= ref["hits_hi"]).all(), f"{what}: hits outside the bracket"
    got = wsum.astype(np.float64) * CR.Q
    err = np.abs(got - ref["wsum"])
    bound = 1e-4 * ref["wsum"] + ref["pairs"] * CR.Q
    assert (err <= bound).all(), f"{what}: weight_sum off by {err.max():.3g} (worst excess {np.max(err - bound):.3g})"
    dev = np.abs(wmax.astype(np.float64) - ref["wmax"]).max() / ref["wmax"].max()
    print(f"{what}: weight_max deviation / max(want) = {dev:.3g}; weight_sum worst relative {np.max(err / np.maximum(ref['wsum'], 1e-30)):.3g}")
    assert dev <= WMAX_TOL, f"{what}: weight_max off by {dev:.3g} of its largest value"


@pytest.mark.parametrize("case", CASES)
def test_against_the_reference(device, case):
    s = scene(case)
    assert s.bad.mean() <= 0.12, "too much of the frame is masked"
    assert int(s.counts.max()) > 64 and sum(int(st.sum()) for _, _, st in s.dec["steps"]) > 1000
    r = Run(device, s)
    try:
        for min_weight in (0.0, MIN_WEIGHT):
            ref = s.ref(min_weight)
            r.fill(*PRIOR)
            assert r.call(s.mask, min_weight) == 0
            hits, wmax, wsum = r.read()
            untouched = ref["pairs"] == 0
            assert untouched.any() and (~untouched).sum() > 100
            # splats in no unmasked pair keep their prior bytes
            assert (hits[untouched] == PRIOR[0]).all() and (wsum[untouched] == PRIOR[2]).all()
            assert np.array_equal(wmax[untouched].view(np.uint32), np.full(untouched.sum(), PRIOR[1], np.float32).view(np.uint32))
            assert (wmax[~untouched] > PRIOR[1]).all()
            wmax = np.where(untouched, np.float32(0), wmax)
            check_against(ref, (hits - PRIOR[0]).astype(np.int64), wmax, wsum - np.uint64(PRIOR[2]), min_weight == 0.0,
                          f"{case[:3]} min_weight={min_weight}")
            if min_weight:
                assert (ref["hits_hi"] < ref["pairs"]).any()  # (the threshold cuts something)
    finally:
        r.destroy()


def test_outputs_are_optional_one_by_one(device):
    s = scene(CASES[0])
    r = Run(device, s)
    try:
        r.fill()
        assert r.call(s.mask) == 0
        full = r.read()
        for k in range(3):
            r.fill(*PRIOR)
            assert r.call(s.mask, outs=tuple(j == k for j in range(3))) == 0
            got = r.read()
            for j in range(3):
                if j != k:
                    assert (got[j] == np.asarray(PRIOR[j], got[j].dtype)).all()  # a NULL output's buffer is not touched
            if k == 1:
                assert np.array_equal(np.maximum(full[1], PRIOR[1]), got[1])
            else:
                assert np.array_equal(full[k] + np.asarray(PRIOR[k], full[k].dtype), got[k])
    finally:
        r.destroy()


def test_accumulates_over_views(device):
    """Two calls, two cameras, the same buffers: the element-wise max, the sum of sums and the sum of hits."""
    case = CASES[1]
    a, b = scene(case), scene(case, "second")
    assert b.bad.mean() <= 0.12 and not np.array_equal(a.counts, b.counts)
    ra, rb = Run(device, a), Run(device, b)
    try:
        ra.fill()
        assert ra.call(a.mask, MIN_WEIGHT) == 0
        first = ra.read()
        rb.out, spare = ra.out, rb.out  # the second view adds into the first's buffers
        assert rb.call(b.mask, MIN_WEIGHT) == 0
        hits, wmax, wsum = rb.read()
        rb.out = spare
        rb.fill()
        assert rb.call(b.mask, MIN_WEIGHT) == 0
        second = rb.read()
    finally:
        ra.destroy()
        rb.destroy()
    # exactly: integer sums and a maximum of the two single-view results
    assert np.array_equal(hits, first[0] + second[0]) and np.array_equal(wsum, first[2] + second[2])
    assert np.array_equal(wmax, np.maximum(first[1], second[1]))
    fa, fb = a.ref(MIN_WEIGHT), b.ref(MIN_WEIGHT)
    both = dict(hits_lo=fa["hits_lo"] + fb["hits_lo"], hits_hi=fa["hits_hi"] + fb["hits_hi"], pairs=fa["pairs"] + fb["pairs"],
                wsum=fa["wsum"] + fb["wsum"], wmax=np.maximum(fa["wmax"], fb["wmax"]))
    check_against(both, hits.astype(np.int64), wmax, wsum, False, "two views")


def test_bit_reproducible(device):
    s = scene(CASES[1])
    r = Run(device, s)
    try:
        runs = []
        for _ in range(2):
            r.fill(*PRIOR)
            assert r.call(s.mask, MIN_WEIGHT) == 0
            runs.append(r.read())
    finally:
        r.destroy()
    for x, y in zip(*runs):
        assert np.array_equal(x.view(np.uint8), y.view(np.uint8))


def test_fractional_mask(device):
    """pixel_weight 0.5 (0 on the rim / near pixels), with NaN at a few pixels (it stands for 0) and 2.0 at a few (for 1)."""
    s = scene(CASES[2])
    rng = np.random.default_rng(5)
    good = np.flatnonzero(~s.bad.reshape(-1))
    pick = rng.choice(good, 60, replace=False)
    mask = np.where(s.bad, 0.0, 0.5).astype(np.float32).reshape(-1)
    clamped = mask.copy()
    mask[pick[:30]], clamped[pick[:30]] = np.nan, 0.0
    mask[pick[30:]], clamped[pick[30:]] = 2.0, 1.0
    mask[np.flatnonzero(s.bad.reshape(-1))[:5]] = -3.0  # (negative: 0, as these pixels already are)
    r = Run(device, s)
    try:
        for min_weight in (0.0, MIN_WEIGHT):
            ref = CR.contribution(s.dec, s.n, s.w, s.h, clamped.reshape(s.h, s.w), min_weight)
            r.fill()
            assert r.call(mask.reshape(s.h, s.w), min_weight) == 0
            hits, wmax, wsum = r.read()
            check_against(ref, hits.astype(np.int64), wmax, wsum, min_weight == 0.0, f"fractional mask, min_weight={min_weight}")
    finally:
        r.destroy()


def aov_alpha_sum(device, s):
    fr = TD.Frame(device, s.rec, s.col, s.counts, s.offsets, s.idx, s.w, s.h)
    try:
        _, alpha = fr.forward(want_alpha=True)
    finally:
        fr.destroy()
    return float(alpha.astype(np.float64).sum())


def alpha_cross_check(device, s, what):
    """Without a mask: sum_i weight_sum_i 2^-24 = sum_px alpha of splat_composite_aov on the same ctx (per pixel sum_i w_i = 1 - T_L)."""
    r = Run(device, s)
    try:
        r.fill()
        assert r.call() == 0
        hits, _, wsum = r.read()
    finally:
        r.destroy()
    want = aov_alpha_sum(device, s)
    got = float(wsum.astype(np.float64).sum() * CR.Q)
    pairs = int(hits.astype(np.int64).sum())
    print(f"{what}: sum of weights {got:.6f}, sum of alpha {want:.6f}, pairs {pairs}")
    assert pairs > 10000 and abs(got - want) <= pairs * 2.0 ** -25 + 1e-5 * want, f"{what}: {got} against {want}"
    return wsum


@pytest.mark.parametrize("case", CASES)
def test_against_the_alpha_aov_and_the_backward(device, case):
    s = scene(case)
    wsum = alpha_cross_check(device, s, str(case[:3]))
    # the colour column of the backward with an upstream of (1, 0, 0, 0) is the same sum, in float atomics
    g = np.zeros((s.h, s.w, 4), np.float32)
    g[..., 0] = 1.0
    rc, _, gcol = TG.composite_backward(device, s.rec, s.col, s.counts, s.offsets, s.idx, s.w, s.h, g)
    assert rc == 0
    e = TG.rel_l2(wsum.astype(np.float64) * CR.Q, gcol[:, 0].astype(np.float64))
    assert e <= 1e-4, f"weight_sum against the backward's colour column: relative L2 {e:.3g}"


@pytest.mark.parametrize("kernel", [0, 1])
def test_follows_the_forward_update_order(device, kernel):
    """The weights are formed in the operation order of the kernel that draws the frame (k_composite | k_composite_px, forced
    as tests/test_gpu_grad_decisions.py forces them): under each, the summed weights are that forward's summed alpha."""
    TD.with_kernel(device, kernel)
    try:
        assert TD.route_order(kernel, 160, 120) == ("px" if kernel else "quadrant")
        alpha_cross_check(device, scene(CASES[1]), f"kernel {kernel}")
    finally:
        TD.with_kernel(device, -1)


def test_rejections(device):
    s = scene(CASES[0])
    r = Run(device, s)
    try:
        r.fill(*PRIOR)
        before = r.read()
        assert s.h > 16  # (more than one tile row: a partial range exists)
        bad = [dict(cfg=TG.cfg(footprint=_lib.FOOTPRINT_ISOTROPIC)), dict(cfg=TG.cfg(tile_row1=1)), dict(cfg=TG.cfg(tile_row0=1)),
               dict(outs=(False, False, False)), dict(min_weight=-0.5), dict(min_weight=float("nan")),
               dict(offsets=(2, 0, 0)), dict(offsets=(0, 2, 0)), dict(offsets=(0, 0, 4)), dict(rec_offset=8), dict(pw_offset=2)]
        for kw in bad:
            kw.setdefault("mask", s.mask)
            assert r.call(**kw) == INVALID, kw
        after = r.read()
        for x, y in zip(before, after):
            assert np.array_equal(x.view(np.uint8), y.view(np.uint8))  # nothing was launched
        # n = 0: success, nothing launched
        assert device.lib.splat_composite_contribution(device.ctx, C.byref(TG.cfg()), r.bufs[1].ptr, 1, r.bufs[0].ptr, r.bufs[2].ptr, r.bufs[3].ptr,
                                                       r.bufs[4].ptr, s.w, s.h, None, 0.0, 0, r.out[0].ptr, None, None) == 0
    finally:
        r.destroy()
