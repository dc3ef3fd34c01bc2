"""The band projector's reach cull (project.hip: cannot_reach_band), restated in NumPy float32, against the oracle's exact
tile ranges.

A strict band frame of tile rows [row0, row1) does not project a splat that cannot_reach_band rejects: its record is not
written and no list of the band contains it.  That is right only if every rejected splat's exact tile range (the oracle's
record through tile_range) misses the band.  This file checks the bound itself — not the kernel, which
tests/test_gpu_band_reach.py holds to the oracle's lists — over the adversarial band-edge scenes of tests/band_edge.py and a
seeded random sweep of about 10^6 splats.

The kernel evaluates the bound with the hardware reciprocal and square root (v_rcp_f32, v_sqrt_f32: within 1 ulp).  The
restatement brackets them: every square root and the reciprocal of the denominator are taken 1 ulp low (the bound only
shrinks with each of them), and the reciprocal of c_w, which moves the centre as well as the reach, 1 ulp low, exact and
1 ulp high; a splat counts as rejected if any of those evaluations rejects it.
"""
import math

import numpy as np
import pytest

from oracle import oracle as O
from tests import band_edge as B

F = np.float32


def _down(x):
    return np.nextafter(x, F(-np.inf)).astype(F)


def _up(x):
    return np.nextafter(x, F(np.inf)).astype(F)


def cull_rejects(u, props, normals, tile, row0, row1, disc, hw_ulps=True):
    """cannot_reach_band<DISC> with its caller's radius (|radius|, for discs scaled by max(1, 1.001 |n|)), operation for
    operation in f32.  hw_ulps: the least favourable of the bracketed hardware results (see the module docstring);
    otherwise correctly rounded ones."""
    u = np.asarray(u, F)
    m = u[:16]
    x, y, z, rad = (np.ascontiguousarray(props[:, k], F) for k in range(4))
    lo = _down if hw_ulps else (lambda v: v)
    with np.errstate(all="ignore"):
        r = np.abs(rad)
        if disc:
            nr = np.asarray(normals, F)
            nn = (nr[:, 0] * nr[:, 0] + nr[:, 1] * nr[:, 1]) + nr[:, 2] * nr[:, 2]
            r = r * np.fmax(F(1.0), F(1.001) * lo(np.sqrt(nn)))
        cx = ((m[0] * x + m[4] * y) + m[8] * z) + m[12]
        cy = ((m[1] * x + m[5] * y) + m[9] * z) + m[13]
        cw = ((m[3] * x + m[7] * y) + m[11] * z) + m[15]

        def row(i):
            if disc:
                return F(1.001) * lo(np.sqrt(F((m[i] * m[i] + m[i + 4] * m[i + 4]) + m[i + 8] * m[i + 8])))
            return F(max(abs(m[i]), abs(m[i + 4]), abs(m[i + 8])))

        ax, ay, aw = r * row(0), r * row(1), r * row(3)
        den = cw - aw
        doubtful = ~(cw > 0) | ~(den > 0)
        iden = lo(F(1.0) / den)
        rejected = np.zeros(x.shape, bool)
        icws = (_down, lambda v: v, _up) if hw_ulps else (lambda v: v,)
        for adj in icws:
            icw = adj(F(1.0) / cw)
            ndx, ndy = cx * icw, cy * icw
            bx = ((F(0.5) * u[20]) * (ax + np.abs(ndx) * aw)) * iden
            by = ((F(0.5) * u[21]) * (ay + np.abs(ndy) * aw)) * iden
            reach = lo(np.sqrt(bx * bx + by * by)) * (F(1.5) * F(1.001)) + F(1.0)
            scy = ((F(1.0) - ndy) * F(0.5)) * u[21]
            ts = F(tile)
            rej = (scy + reach < F(row0) * ts - F(2.0)) | (scy - reach > F(row1) * ts + F(2.0))
            rejected |= rej & ~doubtful
    return rejected


def _explain(u, props, normals, rec, tile, row0, row1, bad, disc):
    i = int(np.nonzero(bad)[0][0])
    return (f"{int(bad.sum())} splat(s) the oracle bins into tile rows [{row0}, {row1}) at T={tile} are rejected by the reach "
            f"bound; first: #{i} pos/radius {props[i, :4].tolist()} normal {normals[i, :3].tolist()} oracle bounds "
            f"{rec[i, :4].tolist()} (band edges y = {row0 * tile}, {row1 * tile}; screen {int(u[20])}x{int(u[21])}, disc={disc})")


def check_no_band_splat_rejected(u, props, normals, tile, row0, row1, footprint):
    disc = footprint == "disc"
    w, h = int(u[20]), int(u[21])
    rec = B.records(u, props, normals, footprint)
    inside = B.in_band(rec, w, h, tile, row0, row1)
    rej = cull_rejects(u, props, normals, tile, row0, row1, disc)
    bad = inside & rej
    assert not bad.any(), _explain(u, props, normals, rec, tile, row0, row1, bad, disc)
    return rec, inside, rej


# ---- the adversarial scenes ------------------------------------------------------------------------------------------
SCENES = [(cam, aspect, tile) for cam in B.CAMERAS for aspect, tile in ((1.0, 16), (0.2, 24), (5.0, 64), (1.6, 16))]


@pytest.mark.parametrize("footprint", ["isotropic", "disc"])
@pytest.mark.parametrize("cam,aspect,tile", SCENES)
def test_band_edge_scenes_keep_every_splat_of_the_band(cam, aspect, tile, footprint):
    w, h = B.screen_for(aspect)
    u = B.make_camera(cam, w, h)
    nty = -(-h // tile)
    kinds = set()
    for k, (row0, row1) in enumerate([(nty // 3, nty // 3 + max(1, nty // 5)), (0, nty // 2), (nty // 2, nty), (1, nty - 1)]):
        props, normals, aim, kind = B.band_edge_scene(u, tile, row0, row1, footprint, seed=k)
        rec, inside, _ = check_no_band_splat_rejected(u, props, normals, tile, row0, row1, footprint)
        # the scene does what it is for: splats on both sides of each inner boundary, from every kind of placement
        for edge, col, which in ((row0 * tile, 3, "row0"), (row1 * tile, 1, "row1")):
            if (which == "row0" and row0 == 0) or (which == "row1" and row1 * tile >= h):
                continue
            sel = aim == which
            assert (np.abs(rec[sel, col] - edge) <= 3.5).sum() >= 40, (which, edge)
            assert inside[sel].any() and (~inside[sel]).any()
            on = sel & (rec[:, col] == F(edge))
            assert on.any() or footprint == "disc", (which, "no record edge exactly on the boundary")
        kinds |= set(kind.tolist())
    want = {"beside", "small", "near-eye", "degenerate"} | ({"off-screen"} if footprint == "isotropic" else set())
    assert want <= kinds, kinds


def test_in_band_is_the_oracles_tile_range():
    """B.in_band (vectorised) against the oracle's own binner: a splat is in the band iff it is in some band tile's list."""
    for cam, aspect, tile in SCENES[::3]:
        w, h = B.screen_for(aspect)
        u = B.make_camera(cam, w, h)
        nty, ntx = -(-h // tile), -(-w // tile)
        row0, row1 = nty // 3, nty // 3 + 2
        for footprint in ("isotropic", "disc"):
            props, normals, _, _ = B.band_edge_scene(u, tile, row0, row1, footprint, seed=3)
            rec = B.records(u, props, normals, footprint)
            counts, offsets, idx = O.bin_sorted(rec, np.arange(rec.shape[0], dtype=np.uint32), w, h, tile)
            lo, hi = int(offsets[row0 * ntx]), int(offsets[row1 * ntx]) if row1 < nty else idx.shape[0]
            want = np.zeros(rec.shape[0], bool)
            want[idx[lo:hi]] = True
            assert np.array_equal(B.in_band(rec, w, h, tile, row0, row1), want), (cam, footprint)


# ---- the random sweep ------------------------------------------------------------------------------------------------
def random_frame(rng, n):
    """One random camera, screen, tile size and band, and n splats spread over and far beyond the screen, from the eye out."""
    aspect = math.exp(rng.uniform(math.log(0.2), math.log(5.0)))
    h = int(rng.integers(16, 1200))
    w = max(1, int(round(h * aspect)))
    cam = dict(target=tuple(rng.uniform(-1, 1, 3)), distance=math.exp(rng.uniform(0, math.log(30))),
               azimuth=rng.uniform(-math.pi, math.pi), elevation=rng.uniform(-1.2, 1.2), fov=rng.uniform(10, 120), aspect=w / h)
    if rng.random() < 0.25:
        cam["azimuth"], cam["elevation"] = float(rng.choice([0, math.pi / 2, math.pi, -math.pi / 2])), 0.0
    vp, eye = O.camera(**cam)
    u = O.uniforms(vp, eye, w, h)
    tile = int(rng.choice([4, 8, 16, 16, 24, 32, 64]))
    nty = -(-h // tile)
    row0 = int(rng.integers(0, nty))
    row1 = int(rng.integers(row0 + 1, nty + 1))
    if row0 == 0 and row1 == nty:
        row1 = max(1, nty - 1)
    M = B._vp(u)
    cw_eye = float(np.abs(M[3, :3]).max())
    sx = rng.uniform(-0.5, 1.5, n) * w
    sy = np.where(rng.random(n) < 0.7, rng.uniform(-0.5, 1.5, n) * h, rng.uniform(-8, 9, n) * h)
    cw = np.exp(rng.uniform(math.log(0.02), math.log(200.0), n))
    pos = B.unproject(u, sx, sy, cw).astype(F)
    # radius: from a tenth of a pixel to past the eye
    rad = (cw / cw_eye * np.exp(rng.uniform(math.log(1e-4), math.log(1.5), n))).astype(F)
    props = np.zeros((n, 8), F)
    props[:, :3], props[:, 3], props[:, 7] = pos, rad * rng.choice([1, -1], n), 1
    nr = rng.standard_normal((n, 3))
    nr *= (np.exp(rng.uniform(math.log(0.1), math.log(4.0), n)) / np.linalg.norm(nr, axis=1))[:, None]
    normals = np.zeros((n, 4), F)
    normals[:, :3], normals[:, 3] = nr, 1
    return u, props, normals, tile, row0, row1


@pytest.mark.parametrize("footprint", ["isotropic", "disc"])
def test_random_sweep_keeps_every_splat_of_the_band_and_rejects_far_ones(footprint):
    rng = np.random.default_rng(20261015 + (footprint == "disc"))
    far_total = far_rejected = inside_total = 0
    for _ in range(64):
        u, props, normals, tile, row0, row1 = random_frame(rng, 8192)
        rec, inside, _ = check_no_band_splat_rejected(u, props, normals, tile, row0, row1, footprint)
        inside_total += int(inside.sum())
        # far from the band: a finite record whose box misses the band's rows by more than its own height and 8 px
        b = rec[:, :4].astype(np.float64)
        with np.errstate(invalid="ignore"):
            gap = np.maximum(row0 * tile - b[:, 3], b[:, 1] - row1 * tile)
            far = np.isfinite(b).all(axis=1) & (b[:, 3] > b[:, 1]) & (gap > (b[:, 3] - b[:, 1]) + 8.0)
        nominal = cull_rejects(u, props, normals, tile, row0, row1, footprint == "disc", hw_ulps=False)
        far_total += int(far.sum())
        far_rejected += int((far & nominal).sum())
    assert inside_total > 20000
    # a bound that keeps everything would pass the first assertion: it must also reject most of what is far from the band
    assert far_total > 100000 and far_rejected >= 0.8 * far_total, (far_rejected, far_total)
