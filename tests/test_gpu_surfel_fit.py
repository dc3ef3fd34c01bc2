"""GPU tests of fitting 2D Gaussian surfels: the three surfel entry points of include/splat.h's "Density control and optimiser"
block (splat_density_accumulate_surfel, splat_densify_plan_surfel, splat_densify_geometry_surfel) against the restatement of
tests/surfel_density_ref.py, splat_adam_step and splat_densify_rows on an (n, 2) plane, and splat_renderer_amd.fit.SurfelFit.

Bounds: tests/test_gpu_density.py's header, where the operation is the same (accumulate: the mask and denom exact, grad_accum to
1e-6 relative; plan: rows and counts exact with the inputs 1e-4 away from every threshold; apply: copies bit for bit, new moments
exact zeros, children's log-scales within 1 ulp, children's means within 1e-5 (|mu|_inf + 7 sigma_max); Adam: its bound).  What
is the surfel rule's own: max_radius is bit-equal to the running maximum of the projector's screenRadius, because disc_bounds() is
stated in binary32.  Every test prints the figures it asserts on.
"""
import ctypes as C
import time

import numpy as np
import pytest
import torch

import splat_renderer_amd as sr
from splat_renderer_amd import _lib
from splat_renderer_amd import autograd as AG
from oracle import np_oracle as NO
from oracle import oracle as O
from tests import density_ref as DR
from tests import ellipsoid_ref as ER
from tests import surfel_density_ref as SDR
from tests import surfel_ref as SR
from tests import test_gpu_density as TD  # (its Adam harness: adam_gpu, check_adam, test_adam_mask take any floats_per_row)

pytestmark = pytest.mark.gpu

SENT = np.uint32(0x7FC0BEEF)  # a quiet NaN with a payload: no kernel arithmetic produces these bits
TAIL = 8


def _lib_ctx():
    cx = AG._context(torch.empty(4, device="cuda"))
    return cx.lib, cx.ctx


def _dev(a, offset=0):
    """The array on the device, `offset` floats into a 16-byte aligned buffer, SENT in the TAIL words past it: (view, buffer, offset)."""
    a = np.ascontiguousarray(a)
    words = a.view(np.uint32).reshape(-1)
    buf = np.full(offset + words.size + TAIL, SENT, np.uint32)
    buf[offset:offset + words.size] = words
    t = torch.from_numpy(buf.view(np.int32)).cuda()
    return t[offset:offset + words.size], t, offset


def _ptr(d):
    """The device address of a _dev() plane (an empty view has no data_ptr of its own)."""
    return d[1].data_ptr() + 4 * d[2]


def _host(view, buf, off, dtype, shape):
    raw = buf.cpu().numpy().view(np.uint32)
    assert (raw[:off] == SENT).all() and (raw[off + view.numel():] == SENT).all(), "words outside the plane were written"
    return raw[off:off + view.numel()].view(dtype).reshape(shape).copy()


def _t(a):
    return torch.tensor(np.ascontiguousarray(a, np.float32), device="cuda")


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def ulp32(x):
    x = np.abs(np.asarray(x, np.float32))
    return (np.nextafter(x, np.float32(np.inf)) - x).astype(np.float64)


def camera_u(w, h, **kw):
    vp, eye = O.camera(aspect=w / h, **kw)
    return O.uniforms(vp, eye, w, h)


def unproject(u, ndc, depth):
    """World points at `depth` from the eye on the rays through the NDC points (k, 2)."""
    inv = np.linalg.inv(np.asarray(u[:16], np.float64).reshape(4, 4).T)
    ndc = np.asarray(ndc, np.float64).reshape(-1, 2)
    ends = []
    for z in (0.2, 0.8):
        p = np.concatenate([ndc, np.full((ndc.shape[0], 1), z), np.ones((ndc.shape[0], 1))], axis=1) @ inv.T
        ends.append(p[:, :3] / p[:, 3:4])
    d = ends[1] - ends[0]
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return np.asarray(u[16:19], np.float64) + np.asarray(depth, np.float64).reshape(-1, 1) * d


# ---- accumulate -------------------------------------------------------------------------------------------------------

def accumulate_cloud(n, seed, u):
    """(means (n, 3), scales (n, 2), rotations (n, 4)) float32.  From 257 surfels on: a surfel wholly outside each screen side
    (rows 0-3), one centred on each side (4-7), a zero quaternion and a surfel behind the eye (8, 9), then a quarter of the
    cloud tilted at random close to the eye (steep perspective: large q), the rest a make_cloud cloud."""
    pos, scl, rot, _ = ER.make_cloud(max(n, 16), seed, 1.0, 0.05, degenerate=False)
    pos, scl, rot = pos[:, :3].copy(), scl[:, :2].copy(), rot.copy()
    if n >= 257:
        rng = np.random.default_rng(seed + 100)
        sides = np.array([(-1, 0), (1, 0), (0, -1), (0, 1)], np.float64)
        pos[0:4] = unproject(u, 1.5 * sides, np.full(4, 3.0))
        pos[4:8] = unproject(u, 1.0 * sides, np.full(4, 3.0))
        scl[0:8] = 0.02
        rot[8] = 0
        pos[9] = 2.0 * np.asarray(u[16:19])  # (the eye looks at the origin)
        k = n // 4
        pos[10:10 + k] = unproject(u, rng.uniform(-1.2, 1.2, (k, 2)), rng.uniform(0.25, 0.6, k))
        scl[10:10 + k] = rng.uniform(0.02, 0.06, (k, 2))
    return pos[:n], scl[:n], rot[:n]


@pytest.mark.parametrize("offset", [0, 1])
@pytest.mark.parametrize("n", [1, 257, 4097])
def test_accumulate_surfel(device, n, offset):
    """Two frames (two cameras, width != height) accumulated into the same three planes, which start from non-zero values and lie
    `offset` floats into their buffers with sentinels around them.  The records are splat_project_surfel's."""
    w, h = 200, 120
    lib, ctx = _lib_ctx()
    cams = [camera_u(w, h), camera_u(w, h, azimuth=0.9, elevation=0.3, distance=2.5)]
    pos, scl, rot = accumulate_cloud(n, 3, cams[0])
    rng = np.random.default_rng(n)
    start = [np.abs(rng.normal(0, 1e-3, n)).astype(np.float32), rng.integers(0, 3, n).astype(np.float32),
             np.exp(rng.normal(np.log(3.0), 1.0, n)).astype(np.float32)]
    planes = [_dev(a, offset) for a in start]
    vis_buf = torch.full((n + TAIL,), 0xAB, device="cuda", dtype=torch.uint8)
    ref = [a.astype(np.float64) for a in start]
    run_max = start[2].copy()
    seen = np.zeros(n, bool)
    worst = 0.0
    for f, u in enumerate(cams):
        with torch.no_grad():
            rec, aux = AG.project_surfels(u, _t(pos), _t(scl), _t(rot))
        rec = rec.contiguous()
        grec_h = (rng.standard_normal((n, 8)) * np.exp(rng.normal(-6, 2, (n, 1)))).astype(np.float32)
        grec = _t(grec_h)
        rc = lib.splat_density_accumulate_surfel(ctx, rec.data_ptr(), grec.data_ptr(), n, w, h, *(_ptr(p) for p in planes), vis_buf.data_ptr())
        assert rc == 0, lib.splat_last_error(ctx)
        torch.cuda.synchronize()
        rec_h, proj = rec.cpu().numpy(), aux.projected.cpu().numpy().view(np.float32).reshape(-1, 8)[:n]
        assert np.array_equal(bits(rec_h), bits(SR.records(u, pos, scl, rot)[0])), "the records are not the restatement's"
        mask, *ref = SDR.accumulate(rec_h, grec_h, w, h, *ref)
        on = mask.astype(bool)
        bnd, ok = NO.disc_bounds(rec_h)
        culled = ~(rec_h != 0).any(axis=1)
        out = [ok & (bnd[:, 2] <= 0), ok & (bnd[:, 0] >= w), ok & (bnd[:, 3] <= 0), ok & (bnd[:, 1] >= h)]
        straddle = [on & (bnd[:, 0] < 0), on & (bnd[:, 2] > w), on & (bnd[:, 1] < 0), on & (bnd[:, 3] > h)]
        steep = on & (np.hypot(rec_h[:, 6], rec_h[:, 7]) * proj[:, 5] > 0.5)
        print(f"n={n} offset={offset} frame {f}: {int(on.sum())} visible, {int(culled.sum())} culled, outside per side "
              f"{[int(x.sum()) for x in out]}, straddling {[int(x.sum()) for x in straddle]}, steep {int(steep.sum())}")
        if n >= 257 and f == 0:
            assert culled.sum() >= 2 and all(x.any() for x in out) and all(x.any() for x in straddle) and steep.sum() >= 10
        vis = vis_buf.cpu().numpy()
        assert (vis[n:] == 0xAB).all(), "bytes past the mask were written"
        assert np.array_equal(vis[:n], mask), "the visibility mask differs"
        got = [_host(*p, np.float32, (n,)) for p in planes]
        assert np.array_equal(got[1].astype(np.float64), ref[1]), "denom differs"
        run_max[on] = np.fmax(run_max[on], proj[on, 5])
        assert np.array_equal(bits(got[2]), bits(run_max)), "max_radius is not the running maximum of projected[:, 5]"
        e = float((np.abs(got[0] - ref[0]) / np.where(ref[0] > 0, ref[0], 1)).max())
        worst = max(worst, e)
        assert e <= 1e-6, f"grad_accum relative {e:.3g}"
        seen |= on
    for k in range(3):
        assert np.array_equal(bits(got[k][~seen]), bits(start[k][~seen])), "a plane of a surfel no frame saw changed"
    if n >= 257:
        assert (~seen).any() and seen.any()
    print(f"n={n} offset={offset}: grad_accum worst relative {worst:.3g}; {int((~seen).sum())} surfels seen by neither frame")


# ---- plan and apply ---------------------------------------------------------------------------------------------------

THRESHOLDS = dict(grad_threshold=2e-4, scale_threshold=0.08, min_opacity=0.3)
SCREEN_RADIUS, WORLD_SCALE = 20.0, 0.2
GAP = 1e-4


def plan_cloud(n, seed):
    """A make_cloud cloud as raw surfel parameters with random statistics, every decision quantity at least 1e-3 (relative) from
    its threshold: (means (n, 3), log_scales (n, 2), rotations, logits, grad_accum, denom, max_radius)."""
    rng = np.random.default_rng(seed)
    pos, scl, rot, col = ER.make_cloud(max(n, 1), seed, 1.0, 0.05, degenerate=False)
    pos, scl, rot, col = pos[:n], scl[:n], rot[:n], col[:n]
    ls = np.log(scl[:, :2]).astype(np.float32)
    lo = (np.log(col[:, 3].astype(np.float64)) - np.log1p(-col[:, 3].astype(np.float64)) - 0.3).astype(np.float32)
    dn = rng.integers(0, 4, n).astype(np.float32)
    ga = (dn * np.exp(rng.normal(np.log(2e-4), 1.0, n))).astype(np.float32)
    mr = np.exp(rng.normal(np.log(8.0), 0.8, n)).astype(np.float32)
    for _ in range(3):  # move what is near a threshold away from it
        g, s, o = DR.plan_quantities(ls, lo, ga, dn)
        ga[np.abs(g / THRESHOLDS["grad_threshold"] - 1) < 1e-3] *= np.float32(1.01)
        ls[np.abs(s / THRESHOLDS["scale_threshold"] - 1) < 1e-3] += np.float32(0.01)
        lo[np.abs(o / THRESHOLDS["min_opacity"] - 1) < 1e-3] += np.float32(0.01)
        ls[np.abs(s / WORLD_SCALE - 1) < 1e-3] += np.float32(0.01)
        mr[np.abs(mr / SCREEN_RADIUS - 1) < 1e-3] *= np.float32(1.01)
    return pos[:, :3].copy(), ls, rot.copy(), lo, ga, dn, mr


def assert_gap(ls, lo, ga, dn, mr, cfg):
    g, s, o = DR.plan_quantities(ls, lo, ga, dn)
    pairs = [(g[dn > 0], cfg["grad_threshold"]), (s, cfg["scale_threshold"]), (o, cfg["min_opacity"])]
    if cfg.get("max_screen_radius", 0) > 0:
        pairs.append((mr.astype(np.float64), cfg["max_screen_radius"]))
    if cfg.get("max_world_scale", 0) > 0:
        pairs.append((s, cfg["max_world_scale"]))
    for q, thr in pairs:
        q = q[np.isfinite(q)]
        if np.isfinite(thr) and thr > 0 and q.size:
            assert (np.abs(q / thr - 1) > GAP).all(), "an input sits within 1e-4 of a threshold"


def plan_gpu(ls, lo, ga, dn, mr, seed=0, offset=0, **cfg):
    """splat_densify_plan_surfel on the device: (address of rows, the tensor that owns them, n_out, rows[:n_out], counts, the cfg)."""
    lib, ctx = _lib_ctx()
    n = ls.shape[0]
    assert ls.shape == (n, 2)
    c = _lib.DensifyCfg(cfg["grad_threshold"], cfg["scale_threshold"], cfg["min_opacity"], cfg.get("max_screen_radius", 0.0),
                        cfg.get("max_world_scale", 0.0), cfg.get("max_splats", 0), seed)
    T = [_dev(a, offset) for a in (ls, lo, ga, dn, mr)]
    nbytes = int(lib.splat_densify_plan_workspace_bytes(n))
    ws = torch.empty(nbytes // 4, device="cuda", dtype=torch.int32)
    rows = _dev(np.full(max(2 * n, 1), 0xDEADBEEF, np.uint32))
    n_out, counts = C.c_uint32(12345), (C.c_uint32 * 4)(9, 9, 9, 9)
    rc = lib.splat_densify_plan_surfel(ctx, *(_ptr(t) for t in T), n, C.byref(c), ws.data_ptr(), nbytes, _ptr(rows), C.byref(n_out), counts)
    assert rc == 0, lib.splat_last_error(ctx)
    for t, a in zip(T, (ls, lo, ga, dn, mr)):
        assert np.array_equal(_host(*t, np.uint32, a.shape), a.view(np.uint32)), "an input of the plan was written"
    all_rows = _host(*rows, np.uint32, (max(2 * n, 1),))
    k = int(n_out.value)
    assert (all_rows[k:] == 0xDEADBEEF).all(), "rows past the count were written"
    return _ptr(rows), rows, k, all_rows[:k], dict(zip(("pruned", "kept", "cloned", "split"), (int(x) for x in counts))), c


@pytest.mark.parametrize("n", [0, 1, 4097, 300_000])
def test_plan_surfel_is_the_restatement(device, n):
    pos, ls, rot, lo, ga, dn, mr = plan_cloud(n, 40 + n % 7)
    _, base_counts, _ = SDR.plan(ls, lo, ga, dn, mr, **THRESHOLDS)
    survivors = n - base_counts["pruned"]
    wanted = base_counts["cloned"] + base_counts["split"]
    if n >= 4097:
        for k in ("pruned", "kept", "cloned", "split"):
            assert base_counts[k] >= 0.05 * n, base_counts
    cases = {
        "plain": dict(THRESHOLDS),
        "screen radius and world scale": dict(THRESHOLDS, max_screen_radius=SCREEN_RADIUS, max_world_scale=WORLD_SCALE),
        "cap inactive": dict(THRESHOLDS, max_splats=survivors + wanted + 100),
        "cap cuts": dict(THRESHOLDS, max_splats=max(survivors + wanted // 2, 1)),
        "cap below the survivors": dict(THRESHOLDS, max_splats=max(survivors - 5, 1)),
    }
    for j, (label, cfg) in enumerate(cases.items()):
        assert_gap(ls, lo, ga, dn, mr, cfg)
        want_rows, want_counts, refused = SDR.plan(ls, lo, ga, dn, mr, **cfg)
        _, _, k, rows, counts, _ = plan_gpu(ls, lo, ga, dn, mr, offset=j & 1, **cfg)
        print(f"n={n} {label}: {counts} -> {k} rows ({refused.size} refused)")
        assert counts == want_counts and k == want_rows.shape[0], f"n={n} {label}: {counts} != {want_counts}"
        assert np.array_equal(rows, want_rows), f"n={n} {label}: rows differ"
        if label == "cap cuts" and n >= 4097:
            assert refused.size > 0 and k == cfg["max_splats"]
        if label == "cap below the survivors" and n >= 4097:
            assert k == survivors and refused.size == wanted


def test_plan_surfel_reads_both_columns_and_only_them(device):
    """Everyone alive and wanting more; the larger scale sits in column 0 for the even rows and in column 1 for the odd ones, on
    either side of the scale threshold by halves: a kernel that strides by 3, or reads one column, classifies some row wrongly.
    NaN rows fall where density_ref's test_plan_nan_falls_on_the_safe_side puts them, in either column."""
    n = 4096
    small, large = np.float32(np.log(0.01)), np.float32(np.log(0.5))
    ls = np.full((n, 2), small, np.float32)
    i = np.arange(n)
    big = (i // 2) % 2 == 1
    ls[big & (i % 2 == 0), 0] = large   # l0 > l1
    ls[big & (i % 2 == 1), 1] = large   # l1 > l0
    ls[~big & (i % 2 == 0), 0] = np.float32(np.log(0.02))  # l0 > l1, both under the threshold
    ls[~big & (i % 2 == 1), 1] = np.float32(np.log(0.02))
    lo = np.full(n, 2.0, np.float32)
    ga, dn, mr = np.ones(n, np.float32), np.ones(n, np.float32), np.ones(n, np.float32)
    assert ((ls[:, 0] > ls[:, 1]).sum(), (ls[:, 1] > ls[:, 0]).sum()) == (n // 2, n // 2)
    want_rows, want_counts, _ = SDR.plan(ls, lo, ga, dn, mr, **THRESHOLDS)
    assert want_counts == dict(pruned=0, kept=0, cloned=n // 2, split=n // 2)
    _, _, k, rows, counts, _ = plan_gpu(ls, lo, ga, dn, mr, **THRESHOLDS)
    print(f"alternating columns: {counts}")
    assert counts == want_counts and np.array_equal(rows, want_rows)
    ls[:] = small
    lo[3] = np.nan
    ls[5, 1] = np.nan
    ls[6, 0] = np.nan
    ga[7] = np.nan
    for extra, dead in ((dict(), (3,)), (dict(max_world_scale=1.0), (3, 5, 6))):
        want_rows, want_counts, _ = SDR.plan(ls, lo, ga, dn, mr, **THRESHOLDS, **extra)
        _, _, k, rows, counts, _ = plan_gpu(ls, lo, ga, dn, mr, **THRESHOLDS, **extra)
        kinds = {int(p): sorted(int(x) for x in (rows >> 30)[(rows & DR.PARENT_MASK) == p]) for p in (3, 5, 6, 7, 9)}
        print(f"NaN rows {extra}: {counts}, kinds {kinds}")
        assert counts == want_counts and np.array_equal(rows, want_rows)
        assert kinds == {p: ([] if p in dead else [0] if p == 7 else [0, 1]) for p in (3, 5, 6, 7, 9)}, kinds


def apply_gpu(rows_p, k, c, planes, moments, offset=0):
    """splat_densify_geometry_surfel + splat_densify_rows on the device: ({name: array (k, ...)}, the same for the moments)."""
    lib, ctx = _lib_ctx()
    D = {name: _dev(a, 0 if name == "rotations" else offset) for name, a in planes.items()}
    out = {name: _dev(np.zeros((k,) + a.shape[1:], np.float32), offset) for name, a in planes.items()}
    rc = lib.splat_densify_geometry_surfel(ctx, rows_p, k, _ptr(D["means"]), _ptr(D["log_scales"]), _ptr(D["rotations"]), C.byref(c),
                                           _ptr(out["means"]), _ptr(out["log_scales"]))
    assert rc == 0, lib.splat_last_error(ctx)
    for name in ("rotations", "opacity_logits", "sh"):
        a = planes[name]
        assert lib.splat_densify_rows(ctx, rows_p, k, _ptr(D[name]), _ptr(out[name]), a.shape[1] if a.ndim == 2 else 1, _lib.DENSIFY_COPY) == 0
    mom = {}
    for name, a in moments.items():
        src, dst = _dev(a, offset), _dev(np.full((k,) + a.shape[1:], 3.0, np.float32), offset)
        assert lib.splat_densify_rows(ctx, rows_p, k, _ptr(src), _ptr(dst), a.shape[1] if a.ndim == 2 else 1, _lib.DENSIFY_ZERO_NEW) == 0
        mom[name] = dst
    torch.cuda.synchronize()
    for name, a in planes.items():
        assert np.array_equal(_host(*D[name], np.uint32, a.shape), bits(a)), f"{name}: an input was written"
    got = {name: _host(*out[name], np.float32, (k,) + planes[name].shape[1:]) for name in planes}
    return got, {name: _host(*mom[name], np.float32, (k,) + moments[name].shape[1:]) for name in moments}


@pytest.mark.parametrize("n", [1, 4097, 300_000])
def test_apply_surfel_is_the_restatement(device, n):
    pos, ls, rot, lo, ga, dn, mr = plan_cloud(n, 40 + n % 7)
    if n == 1:
        ga[:], dn[:], lo[:], ls[:] = 1.0, 1.0, 2.0, np.log(0.3)  # the one surfel is split
    rng = np.random.default_rng(n)
    planes = dict(means=pos, log_scales=ls, rotations=rot, opacity_logits=lo, sh=rng.normal(0, 0.3, (n, 12)).astype(np.float32))
    moments = {name: rng.normal(0, 1, planes[name].shape).astype(np.float32) for name in ("means", "log_scales", "opacity_logits")}
    offset = 1 if n == 4097 else 0
    seed = 0xC0FFEE_0000_0001
    rows_p, _keep, k, rows, counts, c = plan_gpu(ls, lo, ga, dn, mr, seed=seed, **THRESHOLDS)
    got, mom = apply_gpu(rows_p, k, c, planes, moments, offset)
    parent, kind = (rows & DR.PARENT_MASK).astype(np.int64), rows >> 30
    copies, children = kind <= 1, kind >= 2
    assert got["log_scales"].shape == (k, 2)
    for name in planes:
        want = DR.apply_rows(rows, planes[name])
        sel = copies if name in ("means", "log_scales") else slice(None)
        assert np.array_equal(bits(got[name][sel]), bits(want[sel])), f"{name}: a copied row differs"
    for name in moments:
        wm = DR.apply_rows(rows, moments[name], zero_new=True)
        assert np.array_equal(bits(mom[name]), bits(wm)), f"{name}: moments differ"
        assert not bits(mom[name][kind != 0]).any(), f"{name}: a new row's moment is not an exact zero"
    if n >= 4097:
        assert counts["split"] >= 0.05 * n and counts["cloned"] >= 0.05 * n
    assert children.any()
    ref_mu, ref_ls = SDR.apply_geometry(rows, pos, ls, rot, seed)
    e_ls = float((np.abs(got["log_scales"][children] - ref_ls[children]) / ulp32(ref_ls[children])).max())
    sig = np.exp(ls.astype(np.float64))[parent[children]].max(axis=1)
    bound = 1e-5 * (np.abs(pos.astype(np.float64))[parent[children]].max(axis=1) + 7 * sig)
    e_mu = float((np.abs(got["means"][children] - ref_mu[children]).max(axis=1) / bound).max())
    normal = DR.rotation_matrices(rot[parent[children]])[:, :, 2]
    off_plane = np.abs(((got["means"][children].astype(np.float64) - pos[parent[children]]) * normal).sum(axis=1))
    e_pl = float((off_plane / bound).max())
    moved = np.abs(got["means"][children] - pos[parent[children]]).max(axis=1)
    print(f"n={n}: {counts}; children's log-scales {e_ls:.3g} ulp, means {e_mu:.3g} of the bound, |n.(child - mu)| at most "
          f"{float(off_plane.max()):.3g} = {e_pl:.3g} of the bound, median |child - parent| / sigma {float(np.median(moved / sig)):.3g}")
    assert e_ls <= 1.0, f"children's log-scales are {e_ls:.3g} ulp from log sigma - log 1.6"
    assert e_mu <= 1.0, f"children's means are {e_mu:.3g} of the bound from the restatement"
    assert e_pl <= 1.0, f"children leave the parent's plane by {e_pl:.3g} of the bound"
    # the same seed gives the same bits, another seed other children (and the same copies)
    again, _ = apply_gpu(rows_p, k, c, planes, {}, offset)
    assert all(np.array_equal(bits(again[name]), bits(got[name])) for name in planes)
    c2 = _lib.DensifyCfg(c.grad_threshold, c.scale_threshold, c.min_opacity, 0.0, 0.0, 0, seed + 1)
    other, _ = apply_gpu(rows_p, k, c2, planes, {}, offset)
    assert np.array_equal(bits(other["means"][copies]), bits(got["means"][copies]))
    assert np.array_equal(bits(other["log_scales"]), bits(got["log_scales"]))
    assert (np.abs(other["means"][children] - got["means"][children]).max(axis=1) > 0).mean() > 0.99


# ---- Adam on an (n, 2) plane --------------------------------------------------------------------------------------------

@pytest.mark.parametrize("offset", [0, 1])
@pytest.mark.parametrize("K", [1, 50])
def test_adam_on_a_two_column_plane(device, K, offset):
    """floats_per_row = 2, the log-scale plane of a surfel fit: test_gpu_density's harness and bound."""
    worst = np.zeros(3)
    for rows in (1, 63, 65, 10_007):
        worst = np.maximum(worst, TD.check_adam(rows, 2, K, 2, (5e-3, 5e-3), seed=rows + 2, offset=offset))
    print(f"adam fpr=2 K={K} offset={offset}: worst |dp| / bound {worst[0]:.3g}, m relative {worst[1]:.3g}, v relative {worst[2]:.3g}")


@pytest.mark.parametrize("offset", [0, 1])
def test_adam_mask_on_a_two_column_plane(device, offset):
    TD.test_adam_mask(device, 2, offset)


# ---- rejections -------------------------------------------------------------------------------------------------------

def test_surfel_entry_points_reject_bad_arguments(device):
    """NULL, a misaligned plane, a count at the limit, a workspace one byte short: SPLAT_ERR_INVALID with a message, nothing
    launched (the outputs keep their sentinels).  The limit is n = 2^30 for accumulate and plan; the geometry's count is n_out,
    which reaches 2 n, so its limit is its peer's 2^31."""
    lib, ctx = _lib_ctx()
    n = 64
    filled = lambda shape: np.full(shape, 0.25, np.float32)  # noqa: E731
    rec, grec = _dev(filled((n, 8))), _dev(filled((n, 8)))
    stats = [_dev(filled(n)) for _ in range(3)]
    vis = torch.full((n,), 0xAB, device="cuda", dtype=torch.uint8)
    ls, lo, rot, mu = _dev(filled((n, 2))), _dev(filled(n)), _dev(filled((n, 4))), _dev(filled((n, 3)))
    rows = _dev(np.arange(2 * n, dtype=np.uint32))
    mu_out, ls_out = _dev(filled((2 * n, 3))), _dev(filled((2 * n, 2)))
    c = _lib.DensifyCfg(2e-4, 0.08, 0.3, 0, 0, 0, 0)
    nbytes = int(lib.splat_densify_plan_workspace_bytes(n))
    ws = torch.zeros(nbytes // 4 + 4, device="cuda", dtype=torch.int32)
    n_out, counts = C.c_uint32(), (C.c_uint32 * 4)()

    def refused(rc, what):
        msg = lib.splat_last_error(ctx)
        assert rc == -1 and msg, f"{what}: rc {rc}, message {msg!r}"
        print(f"{what}: {msg.decode()}")

    def acc(**kw):
        a = dict(rec=_ptr(rec), grec=_ptr(grec), n=n, ga=_ptr(stats[0]), dn=_ptr(stats[1]), mr=_ptr(stats[2]), vis=vis.data_ptr())
        a.update(kw)
        return lib.splat_density_accumulate_surfel(ctx, a["rec"], a["grec"], a["n"], 64, 48, a["ga"], a["dn"], a["mr"], a["vis"])
    refused(acc(rec=None), "accumulate: NULL records")
    refused(acc(vis=None), "accumulate: NULL mask")
    refused(acc(rec=_ptr(rec) + 4), "accumulate: misaligned records")
    refused(acc(ga=_ptr(stats[0]) + 2), "accumulate: misaligned grad_accum")
    refused(acc(n=1 << 30), "accumulate: n = 2^30")
    assert acc(n=0, rec=None) == 0

    def plan(**kw):
        a = dict(ls=_ptr(ls), lo=_ptr(lo), n=n, ws=ws.data_ptr(), nbytes=nbytes, rows=_ptr(rows))
        a.update(kw)
        return lib.splat_densify_plan_surfel(ctx, a["ls"], a["lo"], _ptr(stats[0]), _ptr(stats[1]), _ptr(stats[2]), a["n"], C.byref(c), a["ws"],
                                             a["nbytes"], a["rows"], C.byref(n_out), counts)
    refused(plan(ls=None), "plan: NULL log_scales")
    refused(plan(ls=_ptr(ls) + 2), "plan: misaligned log_scales")
    refused(plan(ws=ws.data_ptr() + 4), "plan: misaligned workspace")
    refused(plan(n=1 << 30, nbytes=1 << 40), "plan: n = 2^30")
    refused(plan(nbytes=nbytes - 1), "plan: a workspace one byte short")
    assert plan(n=0, ls=None) == 0

    def geo(**kw):
        a = dict(rows=_ptr(rows), k=2 * n, mu=_ptr(mu), ls=_ptr(ls), rot=_ptr(rot), mo=_ptr(mu_out), lso=_ptr(ls_out))
        a.update(kw)
        return lib.splat_densify_geometry_surfel(ctx, a["rows"], a["k"], a["mu"], a["ls"], a["rot"], C.byref(c), a["mo"], a["lso"])
    refused(geo(mu=None), "geometry: NULL means")
    refused(geo(ls=_ptr(ls) + 2), "geometry: misaligned log_scales")
    refused(geo(rot=_ptr(rot) + 4), "geometry: misaligned rotations")
    refused(geo(k=1 << 31), "geometry: n_out = 2^31")
    refused(geo(mo=_ptr(mu)), "geometry: in place")
    assert geo(k=0, mu=None) == 0
    torch.cuda.synchronize()
    for plane, shape in ((stats[0], (n,)), (stats[1], (n,)), (stats[2], (n,)), (mu_out, (2 * n, 3)), (ls_out, (2 * n, 2))):
        assert (_host(*plane, np.float32, shape) == 0.25).all(), "a refused call wrote an output"
    assert np.array_equal(_host(*rows, np.uint32, (2 * n,)), np.arange(2 * n, dtype=np.uint32)) and (vis.cpu().numpy() == 0xAB).all()


# ---- SurfelFit ----------------------------------------------------------------------------------------------------------

def small_fit(n, seed, degree=1, off_screen=0, u=None, **kw):
    """A SurfelFit of a well-conditioned cloud (test_gpu_surfel's scene: spread 0.5, scales about 0.08) with random SH; the first
    `off_screen` surfels moved past the screen's sides."""
    pos, scl, rot, col = ER.make_cloud(n, seed, 0.5, 0.08, degenerate=False)
    pos = pos[:, :3].copy()
    if off_screen:
        rng = np.random.default_rng(seed)
        ndc = rng.uniform(1.6, 2.0, (off_screen, 2)) * rng.choice([-1.0, 1.0], (off_screen, 2))
        pos[:off_screen] = unproject(u, ndc, np.full(off_screen, 3.0))
        scl[:off_screen] = 0.02
    sh = np.random.default_rng(seed + 1).normal(0, 0.3, (n, (degree + 1) ** 2, 3)).astype(np.float32)
    sh[:, 0] = (col[:, :3] - 0.5) / ER.SH_C0
    return sr.SurfelFit(_t(pos), _t(scl[:, :2]), _t(rot), _t(col[:, 3]).clamp(0.05, 0.95), _t(sh), **kw), (pos, scl, rot)


def objective(out, target, u):
    rgb, alpha, depth, dist, nmap = out
    return (AG.photometric_loss(rgb, target) + 0.05 * AG.normal_consistency_loss(nmap, depth, u, weight=alpha.detach(), depth_kind="z")
            + 100.0 * dist.mean())


def test_surfel_fit_render_is_render_surfels(device):
    """fit.render(return_depth, normals, distortion) returns the bits of autograd.render_surfels called by hand on the activated
    parameters, and after backward() of the whole 2DGS objective the five planes hold the hand-made call's gradients to the order
    of the atomic sums: relative L2 <= 1e-4 per plane, the bound tests/test_gpu_surfel.py::_check_chain holds render_surfels'
    parameter gradients to (against float64 there), on the rows it keeps: cond(J) <= 100 for means, scales and rotations."""
    n, w, h, near, far = 300, 64, 48, 0.5, 10.0
    u = camera_u(w, h)
    fit, (pos, scl, rot) = small_fit(n, 41)
    assert fit.log_scales.shape == (n, 2) and fit.degree == 1 and fit.n == n
    target = torch.rand((h, w, 3), device="cuda", generator=torch.Generator(device="cuda").manual_seed(2))
    out = fit.render(u, w, h, return_depth=True, normals=True, distortion=(near, far))
    hand = {k: getattr(fit, k).detach().clone().requires_grad_() for k in ("means", "log_scales", "rotations", "opacity_logits", "sh")}
    feats = AG.surfel_normals(hand["rotations"], hand["means"], u[16:19])
    want = AG.render_surfels(u, hand["means"], torch.exp(hand["log_scales"]), hand["rotations"], torch.sigmoid(hand["opacity_logits"]),
                             sh=hand["sh"], width=w, height=h, degree=1, return_depth=True, features=feats, distortion=(near, far))
    assert len(out) == len(want) == 5
    for name, a, b in zip(("rgb", "alpha", "depth", "distortion", "normals"), out, want):
        assert a.shape == b.shape and torch.equal(a, b), f"{name}: SurfelFit.render differs from render_surfels"
    assert out[4].shape == (h, w, 3) and float(out[1].detach().max()) > 0.5
    objective(out, target, u).backward()
    objective(want, target, u).backward()
    good = SR.geometry64(u, pos, np.concatenate([scl[:, :2], np.zeros((n, 2), np.float32)], axis=1), rot)["cond"] <= 100
    assert good.sum() >= n // 3
    assert fit.log_scales.grad.shape == (n, 2)
    for name in hand:
        got, ref = getattr(fit, name).grad, hand[name].grad
        assert got is not None and torch.isfinite(got).all() and float(got.abs().max()) > 0, name
        rows = torch.as_tensor(good, device="cuda") if name in ("means", "log_scales", "rotations") else slice(None)
        e = float((got[rows].double() - ref[rows].double()).norm() / ref[rows].double().norm())
        print(f"SurfelFit {name}: gradient against the hand-made call, relative L2 {e:.3g}")
        assert e <= 1e-4, f"{name}: relative L2 {e:.3g}"
    assert fit._frame[0].grad is not None and fit._frame[0].grad.shape == (n, 8)
    fit.step()
    with pytest.raises(sr.SplatError, match="normals=True"):
        fit.render(u, w, h, normals=True, features=torch.ones(n, device="cuda"))
    with pytest.raises(sr.SplatError):
        fit.render(torch.tensor(u, requires_grad=True), w, h)
    for name, args in (("update_filter_3d", ([u], w, h)), ("relocate", ()), ("add_new", (100,)), ("inject_noise", ()),
                       ("accumulate_importance", (u, w, h)), ("importance", ()), ("prune_by_importance", ())):
        with pytest.raises(sr.SplatError, match=rf"SurfelFit\.{name}: not built for surfels"):
            getattr(fit, name)(*args)


def test_surfel_fit_sparse_step_leaves_unseen_rows_alone(device):
    n, w, h, off = 300, 64, 48, 40
    u = camera_u(w, h)
    fit, _ = small_fit(n, 43, off_screen=off, u=u)
    target = torch.rand((h, w, 3), device="cuda", generator=torch.Generator(device="cuda").manual_seed(3))
    names = ("means", "log_scales", "rotations", "opacity_logits", "sh")
    for k in range(2):  # (the second step starts from moments that are not zero)
        before = {name: (getattr(fit, name).detach().clone(), fit.m[name].clone(), fit.v[name].clone()) for name in names}
        denom = fit.denom.clone()
        objective(fit.render(u, w, h, return_depth=True, normals=True, distortion=(0.5, 10.0)), target, u).backward()
        fit.step()
        vis = fit.visible.bool()
        assert not vis[:off].any() and int(vis.sum()) > n // 2, "the surfels placed off screen must be invisible"
        assert torch.equal(fit.denom, denom + vis.float())
        changed = {}
        for name in names:
            after = (getattr(fit, name).detach(), fit.m[name], fit.v[name])
            for a, b in zip(before[name], after):
                assert torch.equal(a[~vis], b[~vis]), f"{name}: a row the frame did not see changed"
            changed[name] = float((before[name][0][vis] != after[0][vis]).reshape(int(vis.sum()), -1).any(dim=1).float().mean())
        print(f"step {k + 1}: {int(vis.sum())} of {n} visible; visible rows whose parameters changed: {changed}")
        assert all(c > 0.5 for c in changed.values()), changed


FIT_STEPS, FIT_CAP = 400, 4000


def fit_scene(seed):
    """The target frame of 2 000 surfels at 128 x 128 (ellipsoid_ref.make_cloud read as surfels, its colours as SH of degree 0) and a
    start of 250 of them, perturbed as test_gpu_density.fit_scene perturbs its Gaussians: scales doubled, every parameter moved."""
    n, w, h = 2000, 128, 128
    u = camera_u(w, h)
    pos, scl, rot, col = ER.make_cloud(n, 31, 1.0, 0.04, degenerate=False)
    to_sh = lambda rgb: (rgb - 0.5) / ER.SH_C0  # noqa: E731
    gt = dict(means=_t(pos[:, :3]), scales=_t(scl[:, :2]), rotations=_t(rot), opacity=_t(col[:, 3]).clamp(0.05, 0.95),
              rgb=_t(col[:, :3]).clamp(0.05, 0.95))
    with torch.no_grad():
        target = AG.render_surfels(u, gt["means"], gt["scales"], gt["rotations"], gt["opacity"], sh=to_sh(gt["rgb"]), width=w, height=h)[0].clone()
    g = torch.Generator(device="cuda").manual_seed(seed)
    pick = torch.randperm(n, device="cuda", generator=g)[:250]
    r = lambda shape: torch.randn(shape, device="cuda", generator=g)  # noqa: E731
    start = dict(means=gt["means"][pick] + 0.01 * r((250, 3)),
                 scales=torch.exp(torch.log(2.0 * gt["scales"][pick]) + 0.2 * r((250, 2))),
                 rotations=gt["rotations"][pick] + 0.2 * r((250, 4)),
                 opacity=torch.sigmoid(torch.logit(gt["opacity"][pick]) + 1.0 * r((250,))),
                 sh=to_sh(torch.sigmoid(torch.logit(gt["rgb"][pick]) + 1.0 * r((250, 3)))))
    return u, w, h, target, start


def run_fit(u, w, h, target, start, density_control):
    fit = sr.SurfelFit(start["means"], start["scales"], start["rotations"], start["opacity"], start["sh"])
    counts, events = [fit.n], []
    for step in range(1, FIT_STEPS + 1):
        rgb, _ = fit.render(u, w, h)
        AG.photometric_loss(rgb, target).backward()
        fit.step()
        if density_control and step % 100 == 0 and step <= 300:
            events.append(fit.densify_and_prune(max_splats=FIT_CAP))
            counts.append(fit.n)
            if step == 200:
                fit.reset_opacity(0.01)
    with torch.no_grad():
        rgb, _ = fit.render(u, w, h)
        loss = float(AG.photometric_loss(rgb, target))
    return fit, loss, counts, events


def test_density_control_improves_the_surfel_fit(device, tmp_path):
    """400 steps from 250 surfels, without (A) and with density control (B: densify_and_prune(max_splats=4000) every 100 steps up
    to step 300, one opacity reset), test_gpu_density.test_density_control_improves_the_fit's condition: for each of three seeds
    everything is finite, B's count grew and never exceeded the cap, and B's final photometric loss is not above A's.  No ratio
    is fixed in advance; the losses and counts are printed.  Then the PLY round trip: B's saved file, read by load_surfel_ply and
    drawn by render_surfels, is within 1e-5 of B rendered with exact_activations (that test's comparison (1) and its bound)."""
    t0 = time.time()
    for seed in (1, 2, 3):
        u, w, h, target, start = fit_scene(seed)
        fit_a, loss_a, _, _ = run_fit(u, w, h, target, start, False)
        fit_b, loss_b, counts, events = run_fit(u, w, h, target, start, True)
        print(f"seed {seed}: A (250 surfels, no density control) loss {loss_a:.5f}; B loss {loss_b:.5f}, counts {counts}, events {events}")
        for fit in (fit_a, fit_b):
            assert all(torch.isfinite(p).all() for p in fit.parameters())
            assert all(torch.isfinite(x).all() for x in list(fit.m.values()) + list(fit.v.values()))
        assert np.isfinite(loss_a) and np.isfinite(loss_b)
        assert fit_b.log_scales.shape == (fit_b.n, 2) and fit_b.m["log_scales"].shape == (fit_b.n, 2)
        assert counts[-1] > counts[0] and max(counts) <= FIT_CAP, counts
        path = str(tmp_path / f"surfels{seed}.ply")
        fit_b.save_ply(path)
        g = sr.load_surfel_ply(path)
        assert g["positions"].shape[0] == fit_b.n and g["degree"] == 0 and g["scales"].shape == (fit_b.n, 2)
        with torch.no_grad():
            img = AG.render_surfels(u, _t(g["positions"]), _t(g["scales"]), _t(g["rotations"]), _t(g["opacity"]), sh=_t(g["sh"]),
                                    width=w, height=h)[0]
            fit_b.exact_activations = True  # (read by _activated() at render time)
            rgb_x = fit_b.render(u, w, h)[0]
            fit_b.exact_activations = False
        d = float((img - rgb_x).abs().max())
        print(f"seed {seed}: the saved PLY renders within {d:.3g} of B's parameters under the loader's activations")
        assert d <= 1e-5
        assert loss_b <= loss_a, f"seed {seed}: with density control {loss_b:.5f}, without {loss_a:.5f}"
    elapsed = time.time() - t0
    print(f"surfel fit: {elapsed:.1f} s")
    assert elapsed < 60.0


def test_from_points_starts_as_2dgs_does(device):
    rng = np.random.default_rng(9)
    xyz, rgb = rng.normal(0, 0.5, (500, 3)).astype(np.float32), rng.uniform(0, 1, (500, 3)).astype(np.float32)
    a = sr.SurfelFit.from_points(xyz, rgb, degree=2, rotation_seed=7)
    b = sr.SurfelFit.from_points(xyz, rgb, degree=2, rotation_seed=7)
    c = sr.SurfelFit.from_points(xyz, rgb, degree=2, rotation_seed=8)
    g = sr.GaussianFit.from_points(xyz, rgb, degree=2)
    want = torch.rand((500, 4), generator=torch.Generator(device="cpu").manual_seed(7), dtype=torch.float32)
    assert a.log_scales.shape == (500, 2) and a.sh.shape == (500, 27)
    assert torch.equal(a.rotations.detach().cpu(), want) and torch.equal(a.rotations, b.rotations) and not torch.equal(a.rotations, c.rotations)
    assert float(a.rotations.detach().min()) >= 0 and float(a.rotations.detach().max()) < 1
    assert torch.equal(a.log_scales, g.log_scales[:, :2]) and torch.equal(a.log_scales[:, 0], a.log_scales[:, 1])
    assert torch.equal(a.sh, g.sh) and torch.equal(a.opacity_logits, g.opacity_logits)
    assert torch.equal(g.rotations.detach(), torch.tensor([1.0, 0, 0, 0], device="cuda").repeat(500, 1))


def test_extract_mesh_fuses_the_intersection_depth(device):
    """1 521 flat surfels tiling a tilted plane (normals = the plane's, opacity 0.9), three cameras at 96 x 96, voxel = 1 / 40 of the
    patch: every vertex of the mesh lies within sqrt(3) voxel of the plane.  A vertex sits on a grid or Kuhn-diagonal edge whose
    ends have opposite signs, so within one cell's diagonal of the zero set, and every view's projective distance vanishes exactly
    on the plane, because the intersection depth of a flat surfel is its plane.  The centre-blend depth is not asserted on."""
    m, side, w, h = 39, 1.0, 96, 96
    voxel = side / 40
    nrm = np.array([0.3, 0.2, 1.0])
    nrm /= np.linalg.norm(nrm)
    t0 = np.cross([0.0, 1.0, 0.0], nrm)
    t0 /= np.linalg.norm(t0)
    t1 = np.cross(nrm, t0)
    R = np.stack([t0, t1, nrm], axis=1)
    qw = np.sqrt(1.0 + np.trace(R)) / 2
    quat = np.array([qw, (R[2, 1] - R[1, 2]) / (4 * qw), (R[0, 2] - R[2, 0]) / (4 * qw), (R[1, 0] - R[0, 1]) / (4 * qw)])
    assert np.allclose(DR.rotation_matrices(quat[None])[0], R, atol=1e-12)
    grid = (np.arange(m) + 0.5) / m - 0.5
    a, b = np.meshgrid(grid * side, grid * side, indexing="ij")
    pos = a.reshape(-1, 1) * t0 + b.reshape(-1, 1) * t1
    n = pos.shape[0]
    sh = np.full((n, 1, 3), (0.6 - 0.5) / ER.SH_C0, np.float32)
    fit = sr.SurfelFit(_t(pos), _t(np.full((n, 2), 0.6 * side / m)), _t(np.tile(quat, (n, 1))), _t(np.full(n, 0.9)), _t(sh))
    cams = [camera_u(w, h, distance=2.0, azimuth=az, elevation=el) for az, el in ((0.5, 0.5), (-0.4, 0.3), (0.1, 0.9))]
    assert all(float(np.dot(np.asarray(u[16:19], np.float64), nrm)) > 0.5 for u in cams)
    pending = fit.render(cams[0], w, h)
    frame = fit._frame
    verts, tris, colors = fit.extract_mesh(cams, w, h, voxel)
    assert fit._frame is frame and pending[0].shape == (h, w, 3)
    assert verts.shape[0] > 100 and tris.shape[0] > 100 and colors.shape == verts.shape
    d = (verts.double().cpu().numpy() @ nrm)
    print(f"mesh: {verts.shape[0]} vertices, {tris.shape[0]} triangles; worst |distance to the plane| {float(np.abs(d).max()):.4g} = "
          f"{float(np.abs(d).max()) / voxel:.3g} voxel (bound sqrt(3) = 1.732)")
    assert np.abs(d).max() <= np.sqrt(3.0) * voxel
