"""A NumPy restatement of the auxiliary-output contract of include/splat.h (splat_aov) on the oracle's records and lists.

Per pixel, over the list entries it consumes (nearest first): T_i the transmittance before entry i, g_i the footprint value
(the isotropic Gaussian of oracle.c's composite_rows, or the oriented disc of orc_composite_disc), w_i = T_i g_i; the pixel
stops after the entry at which 1 - T reaches 0.99 (early-out).  Outputs:
  alpha = 1 - T_end (0 where nothing contributed), depth = sum w z / sum w (+inf where sum w = 0), id = the splat index of the
  largest w, the earlier entry on a tie (0xFFFFFFFF where nothing contributed).
The isotropic footprint consumes exactly the entries oracle.composite(..., want_stops=True) reports (pass its `stop`); the
disc's stops are found here in the oracle's binary32 arithmetic.  Also returned, per pixel:
  near      the oracle's `near` pixels (alpha within 2e-5 of 0.99 at some entry: the stop may move by one entry) and, for discs,
            the rim pixels (|d2 - 1| <= 1e-3 at some entry: the discard is a step there);
  id_amb    the two largest weights within 1e-5 relative plus 4e-5 absolute (each weight may be off by the composite's stated
            2e-5 bound): which of them is the largest is not decided by the contract's arithmetic alone;
  tiny      sum w < 1e-30: depth is a ratio of underflowing sums;
  ws, spread  sum w and the largest minus the smallest depth among the contributing entries (for the depth bound).
"""
import numpy as np

from oracle import oracle as O

F = np.float32
U32_NONE = np.uint32(0xFFFFFFFF)


def _iso_g(rec, pxf, pyf):
    inside = ~((pxf < rec[:, 0:1]) | (pxf > rec[:, 2:3]) | (pyf < rec[:, 1:2]) | (pyf > rec[:, 3:4]))
    r = rec[:, 5:6]
    scx, scy = (rec[:, 0:1] + rec[:, 2:3]) * F(0.5), (rec[:, 1:2] + rec[:, 3:4]) * F(0.5)
    ox, oy = pxf - scx, pyf - scy
    with np.errstate(all="ignore"):
        nd = np.sqrt(ox * ox + oy * oy) / r
        g = np.exp(((F(-0.5) * nd) * nd) / F(0.25)).astype(F)
    ok = inside & ~(r < F(0.5))
    return np.where(ok, g, F(0)), np.zeros(g.shape, bool)


def _disc_g(rec, bnd, okb, pxf, pyf):
    dx, dy = pxf - rec[:, 0:1], pyf - rec[:, 1:2]
    with np.errstate(all="ignore"):
        den = F(1) - (rec[:, 6:7] * dx + rec[:, 7:8] * dy)
        nu, nv = rec[:, 2:3] * dx + rec[:, 3:4] * dy, rec[:, 4:5] * dx + rec[:, 5:6] * dy
        uu, vv = nu / den, nv / den
        d2 = uu * uu + vv * vv
        g = np.exp((F(-0.5) * d2) / F(0.16)).astype(F)
    inside = ~((pxf < bnd[:, 0:1]) | (pxf > bnd[:, 2:3]) | (pyf < bnd[:, 1:2]) | (pyf > bnd[:, 3:4]))
    ok = okb[:, None] & inside & (d2 <= F(1))
    rim = okb[:, None] & (np.abs(d2 - F(1)) <= F(1e-3))
    return np.where(ok, g, F(0)), rim


def restate(records, z, indices, counts, offsets, width, height, tile=16, early_out=True, stop=None, disc=False, rows=None):
    """records: (n, 8) ProjectedSplat records (isotropic) or disc records (disc=True); z: (n,) splat depths; the lists as the
    oracle's bin_sorted gives them; stop: oracle.composite's per-pixel entries visited (isotropic).  rows: (r0, r1) tile rows.
    Returns a dict of (H, W) arrays: alpha, depth, id, near, id_amb, tiny, ws, spread, rendered."""
    records = np.asarray(records, F)
    z = np.asarray(z, F)
    ntx, nty = -(-width // tile), -(-height // tile)
    r0, r1 = (0, nty) if rows is None else (rows[0], min(rows[1], nty))
    if disc:
        bnd = np.zeros((records.shape[0], 4), F)
        okb = np.zeros(records.shape[0], bool)
        for s in range(records.shape[0]):
            okb[s], bnd[s] = O.disc_bounds(records[s])
    tiles = np.array([ty * ntx + tx for ty in range(r0, r1) for tx in range(ntx)], np.int64)
    ly, lx = np.divmod(np.arange(tile * tile), tile)
    tx, ty = tiles % ntx, tiles // ntx
    px = tx[:, None] * tile + lx[None, :]
    py = ty[:, None] * tile + ly[None, :]
    inimg = (px < width) & (py < height)
    pxc, pyc = np.minimum(px, width - 1), np.minimum(py, height - 1)
    pxf, pyf = (px.astype(F) + F(0.5)), (py.astype(F) + F(0.5))
    nt, npx = tiles.shape[0], tile * tile
    T = np.ones((nt, npx), F)
    live = inimg.copy()
    zw = np.zeros((nt, npx)); ws = np.zeros((nt, npx))
    w1 = np.zeros((nt, npx), F); w2 = np.zeros((nt, npx), F); idm = np.full((nt, npx), U32_NONE, np.uint32)
    zmin = np.full((nt, npx), np.inf); zmax = np.full((nt, npx), -np.inf)
    near = np.zeros((nt, npx), bool)
    cnt = counts[tiles].astype(np.int64)
    off = offsets[tiles].astype(np.int64)
    pstop = stop[pyc, pxc].astype(np.int64) if stop is not None else None
    for i in range(int(cnt.max()) if nt else 0):
        act = np.nonzero((cnt > i) & live.any(axis=1))[0]
        if act.size == 0:
            break
        s = indices[off[act] + i].astype(np.int64)
        rec = records[s]
        if disc:
            g, rim = _disc_g(rec, bnd[s], okb[s], pxf[act], pyf[act])
            near[act] |= rim & live[act]
        else:
            g, _ = _iso_g(rec, pxf[act], pyf[act])
        lv = live[act] if pstop is None else (inimg[act] & (i < pstop[act]))
        g = np.where(lv, g, F(0))
        Ta = T[act]
        w = Ta * g
        Tn = (Ta * (F(1) - g)).astype(F)
        zi = z[s][:, None]
        zw[act] += w.astype(np.float64) * zi
        ws[act] += w
        pos = w > 0
        zmin[act] = np.where(pos, np.minimum(zmin[act], zi), zmin[act])
        zmax[act] = np.where(pos, np.maximum(zmax[act], zi), zmax[act])
        top = w > w1[act]
        w2[act] = np.where(top, w1[act], np.maximum(w2[act], w))
        w1[act] = np.where(top, w, w1[act])
        idm[act] = np.where(top, s.astype(np.uint32)[:, None], idm[act])
        near[act] |= lv & (np.abs((F(1) - Tn) - F(0.99)) < F(2e-5))
        T[act] = np.where(lv, Tn, Ta)
        if early_out:
            live[act] &= ~(lv & ((F(1) - Tn) >= F(0.99)))
    out = {}
    H, W = height, width

    def scatter(a, fill, dtype):
        img = np.full((H, W), fill, dtype)
        m = inimg
        img[py[m], px[m]] = a[m]
        return img
    with np.errstate(all="ignore"):
        depth = np.where(ws > 0, zw / np.where(ws > 0, ws, 1), np.inf)
    out["alpha"] = scatter((F(1) - T).astype(F), 0, F)
    out["depth"] = scatter(depth, np.inf, np.float64)
    out["id"] = scatter(idm, U32_NONE, np.uint32)
    out["near"] = scatter(near, False, bool)
    out["id_amb"] = scatter((w2 > 0) & ((w1 - w2) <= F(1e-5) * w1 + F(4e-5)), False, bool)
    out["tiny"] = scatter(ws < 1e-30, False, bool)
    out["ws"] = scatter(ws, 0, np.float64)
    out["spread"] = scatter(np.where(ws > 0, zmax - zmin, 0), 0, np.float64)
    out["rendered"] = scatter(np.ones((nt, npx), bool), False, bool)
    return out


def iso_reference(props, normals, u, w, h, tile=16, early_out=True, rows=None):
    """The oracle's pipeline, image and stops, and the restatement on them (isotropic footprint)."""
    from tests.helpers import oracle_pipeline
    ref = oracle_pipeline(props, normals, u, w, h, tile)
    img, img8, _, stop, near = O.composite(O.MODE_FRONT_TO_BACK, early_out, props[:, 4:], normals, ref["proj"], ref["indices"],
                                           ref["counts"], ref["offsets"], w, h, tile=tile, want_stops=True)
    a = restate(ref["proj"], ref["proj"][:, 4], ref["indices"], ref["counts"], ref["offsets"], w, h, tile, early_out, stop=stop,
                rows=rows)
    a["near"] |= near.astype(bool)
    ref.update(img=img, img8=img8, stop=stop, aov=a)
    return ref


def check(got_alpha, got_depth, got_id, a, tol_near, what="", check_depth=True):
    """The test contract: alpha within 2e-5 (tol_near on near pixels), depth within 1e-5 relative where sum w >= 1e-3 and
    1e-3 below — or, where larger, the bound 2e-5 x (depth spread) / sum w that a per-weight error of the composite's stated
    2e-5 gives a weighted mean (|d mean| <= sum |dw_i| |z_i - mean| / sum w) — ids exact, empty pixels exact; ambiguous pixels
    (near; id_amb for ids; tiny for depth) left out of the exact and tight checks."""
    r = a["rendered"]
    near = a["near"]
    empty = r & (a["ws"] == 0) & ~near
    da = np.abs(got_alpha.astype(np.float64) - a["alpha"])
    assert np.all(da[r & ~near] <= 2e-5), f"{what}: alpha off by {da[r & ~near].max()}"
    if near.any():
        assert np.all(da[r & near] <= tol_near), f"{what}: alpha (near) off by {da[r & near].max()}"
    assert np.all(got_alpha[empty] == 0), f"{what}: alpha of an empty pixel"
    assert np.all(got_id[empty] == U32_NONE), f"{what}: id of an empty pixel"
    ok_id = r & ~near & ~a["id_amb"]
    bad = ok_id & (got_id != a["id"])
    assert not bad.any(), f"{what}: {int(bad.sum())} ids differ, first at {np.argwhere(bad)[0]}"
    if check_depth:
        assert np.all(np.isposinf(got_depth[empty])), f"{what}: depth of an empty pixel"
        m = r & ~near & ~a["tiny"] & (a["ws"] > 0)
        ref = a["depth"][m]
        rel = np.where(a["ws"][m] >= 1e-3, 1e-5, 1e-3)
        tol = np.maximum(rel * np.abs(ref), 2e-5 * a["spread"][m] / a["ws"][m])
        dd = np.abs(got_depth[m].astype(np.float64) - ref)
        assert np.all(dd <= tol), f"{what}: depth off by {(dd / np.maximum(tol, 1e-30)).max()} x its bound"
