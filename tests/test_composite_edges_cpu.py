"""The composite oracles (oracle.c's orc_composite and np_oracle.composite) against a float64 evaluation of the reference's
formulas (ComputeShaderRenderer.ts:97-198), on the adversarial record sets of tests/composite_edge.py: box edges on and
one ulp either side of pixel centres, at tile and screen edges and at x >= 2^12; radii at the 0.5 cull; NaN / inf
values; lists ending on and either side of the 32- and 256-entry boundaries; the 0.99 stop reached at a chosen entry;
free boxes.  Both blend modes, early-out on and off.  No GPU.

Tolerance: composite_edge.composite_f64's per-pixel `bound` — a bound, derived per covered entry from the f32 operations
the reference's formulas take (the centre (lo + hi) * 0.5 and the pixel offset carry ulps of |lo| + |hi| and of the
offset, the radius and the exponential a few ulps each), on how far any correct f32 evaluation may be from the float64
one.  At ordinary coordinates it is ~1e-6 per layer; at x ~ 4096 with r = 0.5 the f32 centre alone moves a Gaussian by
up to ~1e-3, and the bound says so.  With early-out on, a pixel whose alpha passes 0.99 within that noise (`near`) may stop
one entry earlier or later; it is held to near_tolerance (what the remaining 1 - 0.99 of the colours can be worth).
"""
import numpy as np
import pytest

from oracle import np_oracle as NP
from oracle import oracle as O
from tests import composite_edge as E

SCENES = E.scenes()
MODES = [O.MODE_FRONT_TO_BACK, O.MODE_REFERENCE_LITERAL]


def sample_pixels(w, h, rng, n=6000):
    """Every pixel of small screens; otherwise the first and last two rows and columns, every tile-edge row and column
    at T = 16 and 64, and n random pixels."""
    if w * h <= 16384:
        py, px = np.mgrid[0:h, 0:w]
        return px.ravel(), py.ravel()
    xs = sorted({0, 1, w - 2, w - 1} | {c for t in (16, 64) for k in range(1, w // t + 1) for c in (k * t - 1, k * t) if c < w})
    ys = sorted({0, 1, h - 2, h - 1} | {c for t in (16, 64) for k in range(1, h // t + 1) for c in (k * t - 1, k * t) if c < h})
    pts = {(x, y) for x in xs for y in range(0, h, 3)} | {(x, y) for y in ys for x in range(0, w, 3)}
    pts |= set(zip(rng.integers(0, w, n).tolist(), rng.integers(0, h, n).tolist()))
    pts = np.array(sorted(pts))
    return pts[:, 0], pts[:, 1]


def check_against_f64(img, want64, bound, near, px, py, mode, early_out, what):
    got = img[py, px, :3].astype(np.float64)
    fin_got, fin_want = np.isfinite(got), np.isfinite(want64)
    assert np.array_equal(fin_got, fin_want), f"{what}: {int((fin_got != fin_want).sum())} channels finite in one and not the other"
    err = np.where(fin_got, np.abs(got - np.where(fin_want, want64, 0.0)), 0.0).max(axis=1)
    tol = np.where(near & early_out, E.near_tolerance(bound, mode), bound)
    bad = err > tol
    if bad.any():
        i = int(np.argmax(err - tol))
        raise AssertionError(f"{what}: {int(bad.sum())} pixels beyond the float64 bound; worst at ({px[i]}, {py[i]}): "
                             f"got {got[i]}, float64 {want64[i]}, bound {tol[i]:.3g}")


@pytest.mark.parametrize("name", sorted(SCENES))
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("early_out", [False, True])
def test_oracles_against_float64(name, mode, early_out):
    sc = SCENES[name]
    rec, _, col, nrm, _ = sc.arrays()
    w, h = sc.w, sc.h
    counts, offsets, idx = E.lists(rec, w, h, 16)
    img, img8, _, stop, onear = O.composite(mode, early_out, col, nrm, rec, idx, counts, offsets, w, h, want_stops=True)
    px, py = sample_pixels(w, h, np.random.default_rng(7))
    want, bound, near = E.composite_f64(mode, early_out, rec, col, nrm, counts, offsets, idx, w, h, 16, px, py)
    check_against_f64(img, want, bound, near | (onear[py, px] > 0), px, py, mode, early_out, f"oracle.c {name}")
    # the NumPy twin: every pixel of the smaller screens (it walks one tile at a time in Python)
    if w * h <= 70000:
        npimg = NP.composite(mode, early_out, col, nrm, rec, idx, counts, offsets, w, h)
        check_against_f64(npimg, want, bound, near | (onear[py, px] > 0), px, py, mode, early_out, f"np_oracle {name}")
        fin = np.isfinite(img)
        assert np.array_equal(fin, np.isfinite(npimg)), f"np_oracle {name}: not finite where oracle.c is, or the reverse"


@pytest.mark.parametrize("mode", MODES)
def test_stop_scenes_stop_where_built(mode):
    """Family c's stop tiles: the centre pixel of tile 2k stops exactly at its list's entry m (1-based m + 1 entries
    visited), the one of tile 2k + 1 (the m-th record one f32 step further out) later."""
    sc = SCENES[f"c_stop{mode}"]
    rec, _, col, nrm, tag = sc.arrays()
    counts, offsets, idx = E.lists(rec, sc.w, sc.h, 16)
    _, _, _, stop, _ = O.composite(mode, True, col, nrm, rec, idx, counts, offsets, sc.w, sc.h, want_u8=False, want_stops=True)
    ntx = sc.w // 16
    built = 0
    for t, m in enumerate(E.STOP_AT):
        for variant in (0, 1):
            if f"stop{m}_{variant}" not in set(tag):
                continue
            built += 1
            tt = 2 * t + variant
            s = int(stop[(tt // ntx) * 16 + 8, (tt % ntx) * 16 + 8])
            assert (s == m + 1) if variant == 0 else (s > m + 1), (m, variant, s)
    assert built == 2 * len(E.STOP_AT)


def test_builders_hit_their_targets():
    """Family a: every aimed box edge is within one f32 step of its target, and the exact hits exist: for every target
    some record's edge equals it bit for bit (ulp-sized targets included)."""
    sc = SCENES["a"]
    rec, compact, _, _, tag = sc.arrays()
    assert compact is not None
    lo_x = rec[tag == "edgex0", 0]
    for col in E.edge_columns(sc.w, (16, 8, 10, 24, 32, 64)):
        for t in E.edge_targets(col):
            assert (lo_x == t).any() or (np.abs(lo_x.astype(np.float64) - t) <= np.spacing(np.float32(abs(t)) * 4)).any(), (col, t)
    assert (lo_x == np.float32(16.5)).any() and (lo_x == np.nextafter(np.float32(16.5), np.float32(0))).any()
