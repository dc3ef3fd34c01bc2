"""GPU tests of 2D Gaussian surfels (SPLAT_FOOTPRINT_SURFEL; include/splat.h, "2D Gaussian surfels") against tests/surfel_ref.py.

Bit-exact: records, ProjectedSplats, keys and clip w of splat_project_surfel; the image under cfg.footprint = SURFEL against
ELLIPSOID over the same records.  Bounds: the image within test_gpu_ellipsoid.py's (rgba32f 1e-4, rgba8 1 LSB off the rim and near
pixels); the intersection depth within 1e-3 |D| + 1e-4 off them; every gradient column within test_gpu_ellipsoid_grad.py's
(relative L2 <= 1e-4, max <= 2e-3 of the column's largest) of the torch float64 restatement, with upstreams zero on rim and near
pixels so that both sides differentiate the same function."""
import ctypes as C
import time

import numpy as np
import pytest
import torch

import splat_renderer_amd as sr
from oracle import np_oracle as NO
from oracle import oracle as O
from splat_renderer_amd import _lib
from tests import ellipsoid_grad_ref as GR
from tests import ellipsoid_ref as ER
from tests import surfel_ref as SR

pytestmark = pytest.mark.gpu

CLOUDS = [(3000, 160, 120, 1, 1.0, 0.03), (500, 64, 64, 3, 0.5, 0.2)]  # n, w, h, seed, spread, scale
TOL, TOL_RIM = 1e-4, 0.02  # (test_gpu_ellipsoid.py's)


def camera_u(w, h):
    vp, eye = O.camera(aspect=w / h)
    return O.uniforms(vp, eye, w, h)


def fptr(u):
    return np.ascontiguousarray(u, np.float32).ctypes.data_as(C.POINTER(C.c_float))


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def cfg(**kw):
    c = dict(mode=_lib.MODE_FRONT_TO_BACK, early_out=1, tile_size=16, tile_row0=0, tile_row1=_lib.U32_MAX,
             record_format=_lib.RECORDS_PROJECTED, prelit=1, footprint=_lib.FOOTPRINT_SURFEL)
    c.update(kw)
    return _lib.CompositeCfg(*c.values())


def rel_l2(got, ref):
    nr = np.linalg.norm(ref)
    return np.linalg.norm(got - ref) / nr if nr > 0 else np.linalg.norm(got)


_scenes = {}


def scene(case):
    """The restated frame of one cloud, computed once: records, clip w, lists, the binary32 composite and its decisions."""
    if case not in _scenes:
        n, w, h, seed, spread, scale = case
        pos, scl, rot, col = ER.make_cloud(n, seed, spread, scale)
        u = camera_u(w, h)
        rec, cw, counts, offsets, idx = SR.lists(u, pos, scl, rot, w, h)
        ref = SR.composite(rec, col, cw, idx, counts, offsets, w, h)
        _scenes[case] = dict(u=u, pos=pos, scl=scl, rot=rot, col=col, rec=rec, cw=cw, counts=counts, offsets=offsets, idx=idx, ref=ref)
    return _scenes[case]


class Frame:
    """The device buffers of a frame's records, colours, z and lists."""

    def __init__(self, d, rec, col, z, counts, offsets, idx):
        self.d, self.n = d, rec.shape[0]
        self.bufs = [d.createBufferFrom(np.ascontiguousarray(a)) for a in
                     (rec, col, z, idx if idx.size else np.zeros(1, np.uint32), counts, offsets)]
        self.rec, self.col, self.z, self.idx, self.cnt, self.off = (b.ptr for b in self.bufs)

    def destroy(self):
        for b in self.bufs:
            b.destroy()

    def image(self, w, h, footprint=_lib.FOOTPRINT_SURFEL, with8=False):
        d = self.d
        out, out8, alpha = d.createBuffer(w * h * 16), d.createBuffer(w * h * 4), d.createBuffer(w * h * 4)
        aov = _lib.Aov(None, alpha.ptr, None)
        _lib.check(d.lib.splat_composite_aov(d.ctx, C.byref(cfg(footprint=footprint)), self.col, 1, None, 1, self.rec, self.idx, self.cnt, self.off,
                                             w, h, out8.ptr, out.ptr, None, C.byref(aov)), d.ctx)
        res = (out.read(np.float32).reshape(h, w, 4), alpha.read(np.float32).reshape(h, w), out8.read(np.uint8).reshape(h, w, 4))
        for b in (out, out8, alpha):
            b.destroy()
        return res if with8 else res[:2]

    def depth(self, w, h, c=None):
        d = self.d
        out, alpha = d.createBuffer(w * h * 4), d.createBuffer(w * h * 4)
        rc = d.lib.splat_composite_surfel_depth(d.ctx, C.byref(c or cfg()), self.col, 1, self.rec, self.idx, self.cnt, self.off, w, h, self.z, 1,
                                                self.n, out.ptr, alpha.ptr)
        res = (rc, out.read(np.float32).reshape(h, w), alpha.read(np.float32).reshape(h, w)) if rc == 0 else (rc, None, None)
        out.destroy()
        alpha.destroy()
        return res

    def backward(self, w, h, g, gd=None, c=None):
        d, n = self.d, self.n
        gb = d.createBufferFrom(np.ascontiguousarray(g, np.float32))
        grec, gcol, gz = d.createBuffer(n * 32), d.createBuffer(n * 16), d.createBuffer(max(n, 1) * 4)
        for b in (grec, gcol, gz):
            b.zero()
        head = (d.ctx, C.byref(c or cfg()), self.col, 1, self.rec, self.idx, self.cnt, self.off, w, h, gb.ptr, n, grec.ptr, gcol.ptr)
        extra = []
        if gd is None:
            rc = d.lib.splat_composite_backward(*head)
        else:
            gdb = d.createBufferFrom(np.ascontiguousarray(gd, np.float32))
            extra.append(gdb)
            rc = d.lib.splat_composite_backward_depth(*head, self.z, 1, gdb.ptr, gz.ptr)
        res = (rc, grec.read(np.float32).reshape(n, 8), gcol.read(np.float32).reshape(n, 4), gz.read(np.float32)[:n]) if rc == 0 else (rc,) + (None,) * 3
        for b in [gb, grec, gcol, gz] + extra:
            b.destroy()
        return res


# ---- projector ---------------------------------------------------------------------------------------------------------------
def run_projector(d, u, pos, scl, rot, n, strides=(1, 1, 1), with_cw=True):
    planes = []
    for a, s in zip((pos, scl, rot), strides):
        wide = np.full((pos.shape[0], 4 * s), 7.0, np.float32)  # (the float4s between the planes' rows are not read)
        wide[:, :4] = a
        planes.append(d.createBufferFrom(wide))
    sorter = sr.RadixSorter(d, max(n, 1))
    padded = sorter.paddedSize
    proj, rec, cw = d.createBuffer(max(n, 1) * 32), d.createBuffer(max(n, 1) * 32), d.createBuffer(max(n, 1) * 4)
    _lib.check(d.lib.splat_project_surfel(d.ctx, fptr(u), planes[0].ptr, strides[0], planes[1].ptr, strides[1], planes[2].ptr, strides[2], n,
                                          proj.ptr, rec.ptr, sorter.getKeysBuffer().ptr, sorter.getPayloadBuffer().ptr, padded,
                                          cw.ptr if with_cw else None), d.ctx)
    out = dict(rec=rec.read(np.float32, n * 8).reshape(n, 8), proj=proj.read(np.float32, n * 8).reshape(n, 8),
               cw=cw.read(np.float32, n), keys=sorter.getKeysBuffer().read(np.uint32), payload=sorter.getPayloadBuffer().read(np.uint32))
    for o in planes + [proj, rec, cw, sorter]:
        o.destroy()
    return out


@pytest.mark.parametrize("case", CLOUDS)
def test_projector_bit_exact(device, case):
    n = case[0]
    s = scene(case)
    rec, proj, keys, cw = SR.project(s["u"], s["pos"], s["scl"], s["rot"])
    kept = (rec != 0).any(axis=1)
    assert not kept[[0, 2, 3, 4, 5, 7]].any() and kept.sum() > n // 2
    for strides in ((1, 1, 1), (3, 1, 3), (1, 3, 1)):
        got = run_projector(device, s["u"], s["pos"], s["scl"], s["rot"], n, strides)
        assert np.array_equal(bits(got["rec"]), bits(rec)), f"records, strides {strides}"
        assert np.array_equal(bits(got["proj"]), bits(proj)), f"projected, strides {strides}"
        assert np.array_equal(bits(got["cw"]), bits(cw)), f"clip w, strides {strides}"
        assert np.array_equal(got["keys"][:n], keys) and (got["keys"][n:] == 0xFFFFFFFF).all()
        assert np.array_equal(got["payload"][:n], np.arange(n, dtype=np.uint32))
        assert (got["rec"][~kept] == 0).all() and (got["cw"][~kept] == 0).all()
    # rows below n do not depend on n; clip_w_out is optional
    for m in (1, 63, 64, 65, 257):
        got = run_projector(device, s["u"], s["pos"], s["scl"], s["rot"], m, with_cw=(m != 64))
        assert np.array_equal(bits(got["rec"]), bits(rec[:m])) and np.array_equal(bits(got["proj"]), bits(proj[:m])), m
        assert np.array_equal(got["keys"][:m], keys[:m]) and (got["keys"][m:] == 0xFFFFFFFF).all(), m


# ---- image -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kernel", ["quadrant", "pixel"])
@pytest.mark.parametrize("case", CLOUDS)
def test_image(device, case, kernel):
    _, w, h = case[:3]
    s = scene(case)
    ref = s["ref"]
    f = Frame(device, s["rec"], s["col"], s["cw"], s["counts"], s["offsets"], s["idx"])
    device.compositeOptions(kernel)
    try:
        img, alpha, img8 = f.image(w, h, with8=True)
        img_e, alpha_e = f.image(w, h, _lib.FOOTPRINT_ELLIPSOID)
    finally:
        device.compositeOptions()
        f.destroy()
    assert np.array_equal(bits(img), bits(img_e)) and np.array_equal(bits(alpha), bits(alpha_e)), "SURFEL and ELLIPSOID draw other bits"
    bad = ref["rim"] | ref["near"]
    dd = np.abs(img[..., :3].astype(np.float64) - ref["img"][..., :3]).max(axis=2)
    print(f"image {kernel} {case[:3]}: max off the rim {dd[~bad].max():.3g}, on it {dd.max():.3g}, bad pixels {bad.sum()}")
    assert dd[~bad].max(initial=0) <= TOL and dd.max() <= TOL_RIM
    want8 = NO.unorm8(ref["img"]).astype(np.int32)
    d8 = np.abs(img8[..., :3].astype(np.int32) - want8[..., :3]).max(axis=2)
    assert d8[~bad].max(initial=0) <= 1
    assert np.abs(alpha - ref["alpha"])[~bad].max() <= TOL


# ---- intersection depth -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kernel", ["quadrant", "pixel"])
@pytest.mark.parametrize("case", CLOUDS)
def test_depth_forward(device, case, kernel):
    _, w, h = case[:3]
    s = scene(case)
    ref = s["ref"]
    f = Frame(device, s["rec"], s["col"], s["cw"], s["counts"], s["offsets"], s["idx"])
    device.compositeOptions(kernel)
    try:
        rc, depth, alpha = f.depth(w, h)
        _, alpha_img = f.image(w, h)
    finally:
        device.compositeOptions()
        f.destroy()
    assert rc == 0
    bad = ref["rim"] | ref["near"]
    want = ref["depth"]
    empty = np.isinf(want)
    assert (~empty).sum() > w * h // 4
    # the sparse cloud leaves pixels nothing reaches (+inf); the dense one covers its whole screen
    assert empty.any() if case is CLOUDS[0] else not empty.any()
    assert np.isposinf(depth[empty & ~bad]).all()
    ok = ~empty & ~bad
    err = np.abs(depth[ok] - want[ok])
    print(f"depth {kernel} {case[:3]}: max err {err.max():.3g} at depth up to {want[ok].max():.3g}")
    assert (err <= 1e-3 * np.abs(want[ok]) + 1e-4).all()
    assert np.abs(alpha - alpha_img)[~bad].max() <= 2e-6  # (its own walk: the image's alpha to rounding)


def test_depth_of_a_grazing_surfel_is_the_ray_plane_depth(device):
    """One large surfel seen at a grazing angle: at every covered pixel D is the clip w of the ray-plane intersection (float64), and
    the centre-blend AOV depth is not."""
    w, h = 96, 64
    u = camera_u(w, h)
    m = np.asarray(u, np.float64)
    rows = m[:16].reshape(4, 4).T
    eye = m[16:19]
    # a plane through the origin whose normal is 80 degrees off the view direction
    view = -eye / np.linalg.norm(eye)
    side = np.cross(view, [0.0, 1.0, 0.0])
    side /= np.linalg.norm(side)
    ang = np.deg2rad(80.0)
    nrm = -np.cos(ang) * view + np.sin(ang) * side
    t0 = np.cross(nrm, [0.0, 1.0, 0.0])
    t0 /= np.linalg.norm(t0)
    t1 = np.cross(nrm, t0)
    R = np.stack([t0, t1, nrm], axis=1)
    if np.linalg.det(R) < 0:
        R[:, 1] = -R[:, 1]
    qw = np.sqrt(max(0.0, 1 + R[0, 0] + R[1, 1] + R[2, 2])) / 2
    quat = np.array([qw, (R[2, 1] - R[1, 2]) / (4 * qw), (R[0, 2] - R[2, 0]) / (4 * qw), (R[1, 0] - R[0, 1]) / (4 * qw)])
    pos = np.array([[0.0, 0.0, 0.0, 1.0]], np.float32)
    scl = np.array([[0.3, 0.3, 0.0, 0.0]], np.float32)
    rot = quat[None, :].astype(np.float32)
    col = np.array([[0.9, 0.5, 0.2, 0.8]], np.float32)
    rec, cw, counts, offsets, idx = SR.lists(u, pos, scl, rot, w, h)
    assert (rec != 0).any()
    ref = SR.composite(rec, col, cw, idx, counts, offsets, w, h)
    geo = SR.geometry64(u, pos, scl, rot)
    f = Frame(device, rec, col, cw, counts, offsets, idx)
    rc, depth, _ = f.depth(w, h)
    # the centre blend: splat_composite_aov_depth's depth with the same z
    d = device
    out, dz = d.createBuffer(w * h * 16), d.createBuffer(w * h * 4)
    aov = _lib.Aov(dz.ptr, None, None)
    _lib.check(d.lib.splat_composite_aov_depth(d.ctx, C.byref(cfg()), f.col, 1, None, 1, f.rec, f.idx, f.cnt, f.off, w, h, None, out.ptr, None,
                                               C.byref(aov), f.z, 1), d.ctx)
    centre = dz.read(np.float32).reshape(h, w)
    out.destroy()
    dz.destroy()
    f.destroy()
    assert rc == 0
    covered = np.isfinite(ref["depth"]) & ~(ref["rim"] | ref["near"])
    assert covered.sum() > 200
    # the analytic clip w: the pixel's ray o + t dir meets the plane (P - p) . n = 0; rays from the inverse of VP
    inv = np.linalg.inv(rows)
    ys, xs = np.nonzero(covered)
    ndc = np.stack([2 * (xs + 0.5) / w - 1, 1 - 2 * (ys + 0.5) / h], 1)
    n64 = np.cross(geo["e0"][0], geo["e1"][0])
    want = np.empty(len(xs))
    for k, (a, b) in enumerate(ndc):
        p0, p1 = inv @ np.array([a, b, 0.0, 1.0]), inv @ np.array([a, b, 0.5, 1.0])
        p0, p1 = p0[:3] / p0[3], p1[:3] / p1[3]
        t = np.dot(pos[0, :3] - p0, n64) / np.dot(p1 - p0, n64)
        want[k] = (rows @ np.append(p0 + t * (p1 - p0), 1.0))[3]
    got = depth[ys, xs].astype(np.float64)
    assert (np.abs(got - want) <= 1e-3 * np.abs(want) + 1e-4).all(), np.abs(got - want).max()
    assert want.max() - want.min() > 0.2  # the plane recedes across the footprint ...
    off = np.abs(centre[ys, xs] - want)
    assert (off > 1e-3 * np.abs(want) + 1e-4).mean() > 0.8 and off.max() > 0.1  # ... and the centre blend is flat


# ---- composite backward, with and without depth ----------------------------------------------------------------------------------
def check_grads(name, got, want, n_cols):
    assert np.isfinite(got).all(), name
    for k in range(n_cols):
        g, wv = (got[:, k], want[:, k]) if n_cols > 1 else (got, want)
        e, mx = rel_l2(g, wv), np.abs(g - wv).max()
        print(f"  {name}[{k}]: relative L2 {e:.3g}, max {mx:.3g} of {np.abs(wv).max():.3g}")
        assert e <= 1e-4, f"{name}[{k}]: relative L2 {e:.3g}"
        assert mx <= 2e-3 * np.abs(wv).max() + 1e-30, f"{name}[{k}]: max {mx:.3g}"


def backward_case(device, rec, col, cw, counts, offsets, idx, w, h, dec, kernel, seed, cache=None):
    """Both backwards of one frame under one drawing kernel against float64 (the reference is computed once per frame: cache)."""
    n = rec.shape[0]
    cache = {} if cache is None else cache
    bad = dec["rim"] | dec["near"]
    g = GR.upstream(w, h, dec["rim"], dec["near"], seed)
    gd = np.random.default_rng(seed + 100).uniform(-1, 1, (h, w)).astype(np.float32)
    gd[bad] = 0
    f = Frame(device, rec, col, cw, counts, offsets, idx)
    device.compositeOptions(kernel)
    try:
        rc0, grec0, gcol0, _ = f.backward(w, h, g)
        rc1, grec1, gcol1, gz1 = f.backward(w, h, g, gd)
    finally:
        device.compositeOptions()
        f.destroy()
    assert rc0 == 0 and rc1 == 0
    reached = np.zeros(n, bool)
    for _pix, s, _stop in dec["steps"]:
        reached[s] = True
    if "want" not in cache:
        cache["want"] = SR.composite_grads(rec, col, dec["steps"], w, h, g) + SR.composite_grads(rec, col, dec["steps"], w, h, g, cw, gd)
    want_rec, want_col = cache["want"][:2]
    check_grads("rec", grec0, want_rec, 8)
    check_grads("col", gcol0, want_col, 4)
    want_rec, want_col, want_z = cache["want"][2:]
    check_grads("depth: rec", grec1, want_rec, 8)
    check_grads("depth: col", gcol1, want_col, 4)
    check_grads("depth: z", gz1, want_z, 1)
    for a in (grec0, gcol0, grec1, gcol1, gz1):
        assert (a[~reached] == 0).all()
    return reached


@pytest.mark.parametrize("kernel", ["quadrant", "pixel"])
@pytest.mark.parametrize("case", CLOUDS)
def test_composite_backward(device, case, kernel):
    _, w, h, seed = case[:4]
    s = scene(case)
    print(f"backward {kernel} {case[:3]}")
    reached = backward_case(device, s["rec"], s["col"], s["cw"], s["counts"], s["offsets"], s["idx"], w, h, s["ref"], kernel, seed,
                            s.setdefault("grads", {}))
    assert reached.sum() > case[0] // 4 and (np.abs(s["rec"][reached, 6:]) > 1e-4).any()


@pytest.mark.parametrize("kernel", ["quadrant", "pixel"])
def test_composite_backward_one_tile_list_lengths(device, kernel):
    """17 x 17: one whole tile, whose list is cut to each chunk edge, and three that the screen's edge cuts (short lists)."""
    w = h = 17
    n = 400
    u = camera_u(w, h)
    pos, scl, rot, col = ER.make_cloud(n, 21, 0.35, 0.1, degenerate=False)
    col[:, 3] *= 0.12  # (faint: no pixel stops before the list's end)
    rec, cw, counts, offsets, idx = SR.lists(u, pos, scl, rot, w, h)
    assert counts[0] >= 129 and (counts[1:] > 0).all()
    for cut in (0, 1, 63, 64, 65, 129):
        c2 = counts.copy()
        c2[0] = cut
        dec = SR.composite(rec, col, cw, idx, c2, offsets, w, h)
        print(f"one tile {kernel}: list of {cut}")
        backward_case(device, rec, col, cw, c2, offsets, idx, w, h, dec, kernel, 21 + cut)


# ---- feature channels -------------------------------------------------------------------------------------------------------------
# test_gpu_features.py's rule, with its margins: the kernel against float64, in units of what a binary32 restatement of the same
# formulas (surfel_ref.composite64 on float32 tensors, never the kernel) loses against float64 on the same frame.  Forward: every
# unmasked (pixel, channel) within MARGIN c_fwd m_px, m_px = sum w |f|, c_fwd the restatement's largest |F32 - F64| / m_px.
# Backward: every reached splat and each of the 9 + K numbers (eight record columns, opacity, K feature columns) within MARGIN
# c_scene m[s, k], m the sum over the splat's pairs of |the pair's term| (float64 autograd with the per-pair rows' gradients
# retained), c_scene the restatement's largest |sum32 - sum64| / m; relative L2 per number at most L2_MARGIN times the restatement's.
MARGIN, L2_MARGIN = 4.0, 8.0
_feature_refs = {}


def feature_case(case, K):
    if (case, K) not in _feature_refs:
        n, w, h, seed = case[:4]
        s = scene(case)
        dec = s["ref"]
        rng = np.random.default_rng(seed * 10 + K)
        f = rng.uniform(-1, 1, (n, K)).astype(np.float32)
        gf = rng.uniform(-1, 1, (h, w, K)).astype(np.float32)
        gf[dec["rim"] | dec["near"]] = 0
        args = (s["rec"], s["col"], f, dec["steps"], w, h)
        F64, m_px = SR.feature_maps(*args)
        F32, _ = SR.feature_maps(*args, dtype=torch.float32)
        g64, m = SR.feature_grads(*args, gf, magnitudes=True)
        g32 = SR.feature_grads(*args, gf, dtype=torch.float32)
        _feature_refs[(case, K)] = dict(f=f, gf=gf, F64=F64, m_px=m_px, F32=F32, g64=g64, g32=g32, m=m)
    return _feature_refs[(case, K)]


def run_features(d, fr, f, w, h, gf=None):
    n, K = f.shape
    fb = d.createBufferFrom(f)
    head = (d.ctx, C.byref(cfg()), fr.col, 1, fr.rec, fr.idx, fr.cnt, fr.off, w, h, fb.ptr, K, K)
    if gf is None:
        out = d.createBuffer(w * h * K * 4)
        rc = d.lib.splat_composite_features(*head, n, out.ptr)
        res = (rc, out.read(np.float32).reshape(h * w, K))
        bufs = [out]
    else:
        gb = d.createBufferFrom(np.ascontiguousarray(gf, np.float32))
        bufs = [gb] + [d.createBuffer(n * k * 4) for k in (8, 4, K)]
        for b in bufs[1:]:
            b.zero()
        rc = d.lib.splat_composite_features_backward(*head, gb.ptr, n, bufs[1].ptr, bufs[2].ptr, bufs[3].ptr, K)
        res = (rc, bufs[1].read(np.float32).reshape(n, 8), bufs[2].read(np.float32).reshape(n, 4), bufs[3].read(np.float32).reshape(n, K))
    for b in [fb] + bufs:
        b.destroy()
    return res


@pytest.mark.parametrize("K", [3, 8])
@pytest.mark.parametrize("kernel", ["quadrant", "pixel"])
@pytest.mark.parametrize("case", CLOUDS)
def test_features_forward(device, case, kernel, K):
    _, w, h = case[:3]
    s, r = scene(case), feature_case(case, K)
    fr = Frame(device, s["rec"], s["col"], s["cw"], s["counts"], s["offsets"], s["idx"])
    device.compositeOptions(kernel)
    try:
        rc, got = run_features(device, fr, r["f"], w, h)
    finally:
        device.compositeOptions()
        fr.destroy()
    assert rc == 0 and np.isfinite(got).all()
    ok = ~(s["ref"]["rim"] | s["ref"]["near"]).reshape(-1)
    has = r["m_px"] > 0
    c_fwd = (np.abs(r["F32"] - r["F64"])[ok][has[ok]] / r["m_px"][ok][has[ok]]).max()
    q = np.abs(got - r["F64"])[ok][has[ok]] / r["m_px"][ok][has[ok]]
    print(f"features forward {kernel} {case[:3]} K={K}: worst err / m_px {q.max() * 2 ** 24:.1f} x 2^-24 against c_fwd {c_fwd * 2 ** 24:.1f} x 2^-24")
    assert (got[ok][~has[ok]] == 0).all()  # nothing contributed: exact 0
    assert (q <= MARGIN * c_fwd).all()


@pytest.mark.parametrize("K", [3, 8])
@pytest.mark.parametrize("kernel", ["quadrant", "pixel"])
@pytest.mark.parametrize("case", CLOUDS)
def test_features_backward(device, case, kernel, K):
    n, w, h = case[:3]
    s, r = scene(case), feature_case(case, K)
    fr = Frame(device, s["rec"], s["col"], s["cw"], s["counts"], s["offsets"], s["idx"])
    device.compositeOptions(kernel)
    try:
        rc, grec, gcol, gfeat = run_features(device, fr, r["f"], w, h, r["gf"])
    finally:
        device.compositeOptions()
        fr.destroy()
    assert rc == 0
    got = np.concatenate([grec, gcol[:, 3:4], gfeat], axis=1).astype(np.float64)
    want, ref32, m = r["g64"], r["g32"], r["m"]
    assert np.isfinite(got).all() and (gcol[:, :3] == 0).all()
    reached = np.zeros(n, bool)
    for _pix, sp, _stop in s["ref"]["steps"]:
        reached[sp] = True
    assert (got[~reached] == 0).all()
    names = ["c.x", "c.y", "B00", "B01", "B10", "B11", "q0", "q1", "opacity"] + [f"f{k}" for k in range(K)]
    has = reached[:, None] & (m > 0)
    c_scene = (np.abs(ref32 - want)[has] / m[has]).max()
    q = np.where(has, np.abs(got - want) / np.where(has, m, 1), 0.0)
    worst = np.unravel_index(np.argmax(q), q.shape)
    print(f"features backward {kernel} {case[:3]} K={K}: worst err / m {q.max() * 2 ** 24:.1f} x 2^-24 (splat {worst[0]}, {names[worst[1]]}) "
          f"against c_scene {c_scene * 2 ** 24:.1f} x 2^-24: ratio {q.max() / c_scene:.2f}")
    assert (got[~has] == 0).all()  # (no term: exact 0)
    assert (q <= MARGIN * c_scene).all(), f"{int((q > MARGIN * c_scene).sum())} (splat, number) sums beyond {MARGIN:g} c_scene m"
    for k, name in enumerate(names):
        l2, l2_ref = rel_l2(got[:, k], want[:, k]), rel_l2(ref32[:, k], want[:, k])
        print(f"  {name}: relative L2 {l2:.3g} (restatement {l2_ref:.3g})")
        assert np.abs(want[:, k]).max() > 0, name
        assert l2 <= L2_MARGIN * l2_ref, f"{name}: relative L2 {l2:.3g} against the restatement's {l2_ref:.3g}"


# ---- projector backward ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CLOUDS)
def test_project_backward(device, case):
    n, w, h, seed = case[:4]
    s = scene(case)
    u, pos, scl, rot = s["u"], s["pos"], s["scl"], s["rot"]
    rng = np.random.default_rng(seed)
    grec = rng.uniform(-1, 1, (n, 8)).astype(np.float32)
    gcw = rng.uniform(-1, 1, n).astype(np.float32)
    d = device
    bufs = [d.createBufferFrom(np.ascontiguousarray(a, np.float32)) for a in (pos, scl, rot, grec, gcw)]
    outs = [d.createBuffer(n * 16) for _ in range(3)]
    res = {}
    for with_cw in (True, False):
        rc = d.lib.splat_project_surfel_backward(d.ctx, fptr(u), bufs[0].ptr, 1, bufs[1].ptr, 1, bufs[2].ptr, 1, n, bufs[3].ptr,
                                                 bufs[4].ptr if with_cw else None, outs[0].ptr, outs[1].ptr, outs[2].ptr)
        assert rc == 0
        res[with_cw] = [o.read(np.float32).reshape(n, 4) for o in outs]
    for b in bufs + outs:
        b.destroy()
    kept = (s["rec"] != 0).any(axis=1)
    geo = SR.geometry64(u, pos, scl, rot)
    good = kept & (geo["cond"] <= 1e4)
    assert good.sum() >= n // 3
    for with_cw in (True, False):
        P = torch.tensor(pos.astype(np.float64), requires_grad=True)
        S = torch.tensor(scl.astype(np.float64), requires_grad=True)
        Q = torch.tensor(rot.astype(np.float64), requires_grad=True)
        rec64, cw64 = SR.records64(u, P, S, Q, kept)
        L = (rec64 * torch.as_tensor(grec.astype(np.float64))).sum()
        if with_cw:
            L = L + (cw64 * torch.as_tensor(gcw.astype(np.float64))).sum()
        L.backward()
        gp, gs, gq = res[with_cw]
        assert all(np.isfinite(a).all() for a in (gp, gs, gq))
        assert (gp[~kept] == 0).all() and (gs[~kept] == 0).all() and (gq[~kept] == 0).all()
        assert (gs[:, 2:] == 0).all() and (gp[:, 3] == 0).all()
        for name, got, want, cols in (("position", gp, P.grad.numpy(), 3), ("scale", gs, S.grad.numpy(), 2), ("rotation", gq, Q.grad.numpy(), 4)):
            for k in range(cols):
                e = rel_l2(got[good, k], want[good, k])
                print(f"project backward (clip w {with_cw}) {name}[{k}]: relative L2 {e:.3g}")
                assert e <= 1e-4, f"{name}[{k}]: relative L2 {e:.3g}"


# ---- refusals --------------------------------------------------------------------------------------------------------------------
def test_entry_points_without_surfel_kernels_refuse_the_footprint(device):
    case = CLOUDS[1]
    n, w, h = case[:3]
    s = scene(case)
    d = device
    f = Frame(d, s["rec"], s["col"], s["cw"], s["counts"], s["offsets"], s["idx"])
    g = d.createBufferFrom(np.zeros((h, w, 4), np.float32))
    big = d.createBuffer(n * 64 + (1 << 20))
    c = cfg()
    calls = {
        "splat_composite_backward_abs": lambda: d.lib.splat_composite_backward_abs(d.ctx, C.byref(c), f.col, 1, f.rec, f.idx, f.cnt, f.off, w, h, g.ptr, n,
                                                                                  big.ptr, big.ptr, None, 0, None, None, big.ptr),
        "splat_composite_backward_det": lambda: d.lib.splat_composite_backward_det(d.ctx, C.byref(c), f.col, 1, f.rec, big.ptr, f.idx, f.cnt, f.off, 0, w,
                                                                                  h, g.ptr, n, big.ptr, big.ptr, None, 0, None, None, big.ptr, 1 << 20),
        "splat_composite_backward_det_abs": lambda: d.lib.splat_composite_backward_det_abs(d.ctx, C.byref(c), f.col, 1, f.rec, big.ptr, f.idx, f.cnt, f.off,
                                                                                          0, w, h, g.ptr, n, big.ptr, big.ptr, None, 0, None, None, big.ptr,
                                                                                          1 << 20, big.ptr),
        "splat_composite_contribution": lambda: d.lib.splat_composite_contribution(d.ctx, C.byref(c), f.col, 1, f.rec, f.idx, f.cnt, f.off, w, h, None, 0.0,
                                                                                  n, big.ptr, None, None),
    }
    try:
        for name, call in calls.items():
            assert call() == -1, name
            msg = d.lib.splat_last_error(d.ctx).decode()
            assert "SPLAT_FOOTPRINT_SURFEL" in msg, (name, msg)
        # the surfel kernels take their own footprint only, and the one configuration
        rc, _, _ = f.depth(w, h, cfg(footprint=_lib.FOOTPRINT_ELLIPSOID))
        assert rc == -1
        for bad in (dict(tile_size=8), dict(early_out=0), dict(tile_row0=1), dict(mode=_lib.MODE_REFERENCE_LITERAL)):
            assert f.depth(w, h, cfg(**bad))[0] == -1, bad
            assert f.backward(w, h, np.zeros((h, w, 4), np.float32), c=cfg(**bad))[0] == -1, bad
    finally:
        for b in (g, big):
            b.destroy()
        f.destroy()


# ---- autograd --------------------------------------------------------------------------------------------------------------------
def _leaf(a):
    return torch.tensor(np.ascontiguousarray(a, np.float32), device="cuda", requires_grad=True)


def _torch_scene(n, seed, spread=0.5, scale=0.1):
    pos, scl, rot, col = ER.make_cloud(n, seed, spread, scale, degenerate=False)
    return pos[:, :3].copy(), scl[:, :3].copy(), rot, col


def test_render_surfels_image_is_the_staged_frame(device):
    from splat_renderer_amd import autograd as AG
    case = CLOUDS[0]
    n, w, h = case[:3]
    s = scene(case)
    f = Frame(device, s["rec"], s["col"], s["cw"], s["counts"], s["offsets"], s["idx"])
    want, want_alpha = f.image(w, h)
    _, want_depth, _ = f.depth(w, h)
    f.destroy()
    with torch.no_grad():
        t = lambda a: torch.tensor(np.ascontiguousarray(a, np.float32), device="cuda")  # noqa: E731
        rgb, alpha, depth = AG.render_surfels(s["u"], t(s["pos"][:, :3]), t(s["scl"][:, :3]), t(s["rot"]), t(s["col"][:, 3]),
                                              colors=t(s["col"][:, :3]), width=w, height=h, return_depth=True)
    torch.cuda.synchronize()
    assert np.array_equal(bits(rgb.cpu().numpy()), bits(want[..., :3]))
    assert np.array_equal(bits(alpha.cpu().numpy()), bits(want_alpha))
    assert np.array_equal(bits(depth.cpu().numpy()), bits(want_depth))


def _chain_reference(u, pos, scl, rot, op, rgb, w, h, g, gd, feats=None, gf=None):
    rec32, cw32, counts, offsets, idx = SR.lists(u, pos, scl, rot, w, h)
    col32 = np.concatenate([rgb, op[:, None]], axis=1).astype(np.float32)
    dec = SR.composite(rec32, col32, cw32, idx, counts, offsets, w, h)
    bad = dec["rim"] | dec["near"]
    g, gd = g.copy(), gd.copy()
    g[bad] = 0
    gd[bad] = 0
    if gf is not None:
        gf = gf.copy()
        gf[bad] = 0
    P = torch.tensor(pos.astype(np.float64), requires_grad=True)
    S = torch.tensor(scl.astype(np.float64), requires_grad=True)
    Q = torch.tensor(rot.astype(np.float64), requires_grad=True)
    OP = torch.tensor(op.astype(np.float64), requires_grad=True)
    RGB = torch.tensor(rgb.astype(np.float64), requires_grad=True)
    kept = (rec32 != 0).any(axis=1)
    rec, cw = SR.records64(u, P, S, Q, kept)
    col = torch.cat([RGB, OP[:, None]], dim=1)
    FT = torch.tensor(feats.astype(np.float64), requires_grad=True) if feats is not None else None
    SR.loss64(SR.composite64(rec, col, dec["steps"], w, h, cw, FT), g, gd, gf).backward()
    want = dict(means=P.grad.numpy(), scales=S.grad.numpy(), rotations=Q.grad.numpy(), opacities=OP.grad.numpy(), colors=RGB.grad.numpy())
    if feats is not None:
        want["features"] = FT.grad.numpy()
        return want, g, gd, gf, dec
    return want, g, gd, dec


def _torch_loss(u, pos, scl, rot, op, rgb, w, h, g, gd, feats=None, gf=None):
    from splat_renderer_amd import autograd as AG
    leaves = dict(means=_leaf(pos), scales=_leaf(scl), rotations=_leaf(rot), opacities=_leaf(op), colors=_leaf(rgb))
    if feats is not None:
        leaves["features"] = _leaf(feats)
    out = AG.render_surfels(u, leaves["means"], leaves["scales"], leaves["rotations"], leaves["opacities"], colors=leaves["colors"],
                            width=w, height=h, return_depth=True, features=leaves.get("features"))
    img, alpha, depth = out[:3]
    gt, gdt = torch.as_tensor(g, device="cuda"), torch.as_tensor(gd, device="cuda")
    has = torch.isfinite(depth)
    loss = (img * gt[..., :3]).sum() + (alpha * gt[..., 3]).sum() + (torch.where(has, depth, torch.zeros_like(depth)) * gdt).sum()
    if feats is not None:
        loss = loss + (out[3] * torch.as_tensor(gf, device="cuda")).sum()
    return leaves, loss


def _check_chain(u, pos, scl, rot, leaves, want):
    # The rows held to the bound: test_gpu_ellipsoid_grad.py keeps cond(Sigma2) <= 1e4, and Sigma2 = J J^T, so cond(J) <= 100 of the
    # surfel's screen Jacobian is the same rule (the record's float32 gradient is amplified by cond(J) on its way to the parameters)
    geo = SR.geometry64(u, pos, scl, rot)
    good = geo["cond"] <= 100
    assert good.sum() >= pos.shape[0] // 3
    for name in [k for k in ("means", "scales", "rotations", "opacities", "colors", "features") if k in leaves]:
        got = leaves[name].grad.detach().cpu().numpy()
        assert np.isfinite(got).all(), name
        rows = good if name in ("means", "scales", "rotations") else np.ones(pos.shape[0], bool)
        e = rel_l2(got[rows].reshape(-1).astype(np.float64), want[name][rows].reshape(-1))
        print(f"render_surfels {name}: relative L2 {e:.3g}")
        assert e <= 1e-4, f"{name}: relative L2 {e:.3g}"
    assert (leaves["scales"].grad[:, 2] == 0).all()


def _upstreams(w, h, seed):
    rng = np.random.default_rng(seed)
    return rng.uniform(-1, 1, (h, w, 4)).astype(np.float32), rng.uniform(-1, 1, (h, w)).astype(np.float32)


def test_render_surfels_gradients(device):
    n, w, h, seed = 200, 64, 48, 41
    u = camera_u(w, h)
    pos, scl, rot, col = _torch_scene(n, seed)
    op, rgb = col[:, 3].copy(), col[:, :3].copy()
    g, gd = _upstreams(w, h, seed)
    # with depth and a feature plane: each surfel's normal (surfel_normals, held fixed here), as 2DGS's normal map blends it
    from splat_renderer_amd import autograd as AG
    feats = AG.surfel_normals(torch.tensor(rot), torch.tensor(pos), u[16:19]).numpy().astype(np.float32)
    gf = np.random.default_rng(seed + 1).uniform(-1, 1, (h, w, 3)).astype(np.float32)
    want, g, gd, gf, _ = _chain_reference(u, pos, scl, rot, op, rgb, w, h, g, gd, feats, gf)
    leaves, loss = _torch_loss(u, pos, scl, rot, op, rgb, w, h, g, gd, feats, gf)
    loss.backward()
    _check_chain(u, pos, scl, rot, leaves, want)


def test_two_forwards_then_two_backwards(device):
    w, h = 64, 48
    u = camera_u(w, h)
    scenes = []
    for seed, n in ((42, 150), (43, 250)):
        pos, scl, rot, col = _torch_scene(n, seed)
        op, rgb = col[:, 3].copy(), col[:, :3].copy()
        g, gd = _upstreams(w, h, seed)
        want, g, gd, _ = _chain_reference(u, pos, scl, rot, op, rgb, w, h, g, gd)
        scenes.append((pos, scl, rot, op, rgb, g, gd, want))
    runs = [_torch_loss(u, *s[:5], w, h, s[5], s[6]) for s in scenes]  # two forwards: the second re-bins the shared binner
    runs[1][1].backward()
    runs[0][1].backward()                                               # the first's lists are rebuilt, not the second's used
    for s, (leaves, _) in zip(scenes, runs):
        _check_chain(u, s[0], s[1], s[2], leaves, s[7])


def test_bad_calls_raise(device):
    from splat_renderer_amd import autograd as AG
    w = h = 64
    u = camera_u(w, h)
    x = torch.zeros((4, 3))
    with pytest.raises(sr.SplatError):
        AG.render_surfels(u, x, x, torch.zeros((4, 4)), torch.zeros(4), colors=x, width=w, height=h)  # CPU tensors
    pos, scl, rot, col = _torch_scene(50, 44)
    t = lambda a: torch.tensor(np.ascontiguousarray(a, np.float32), device="cuda")  # noqa: E731
    rec, aux = AG.project_surfels(u, t(pos), t(scl), t(rot))
    assert aux.footprint == _lib.FOOTPRINT_SURFEL
    for kw in (dict(deterministic=True), dict(absgrad=True)):
        with pytest.raises(sr.SplatError):
            AG.rasterize(rec, t(col), aux, w, h, **kw)
    with pytest.raises(sr.SplatError):
        AG.contribution(rec, t(col), aux, w, h)
    ut = torch.tensor(u, requires_grad=True)
    with pytest.raises(sr.SplatError):
        AG.project_surfels(ut, t(pos), t(scl), t(rot))
    with pytest.raises(sr.SplatError):
        AG.render_surfels(ut, t(pos), t(scl), t(rot), t(col[:, 3]), colors=t(col[:, :3]), width=w, height=h)


def test_fitting_converges(device):
    """400 surfels at 64 x 64: 60 plain Adam steps on image + intersection depth from a perturbed cloud bring the loss down 10x
    (the ratio of test_gpu_ellipsoid_grad.test_fitting_converges)."""
    from splat_renderer_amd import autograd as AG
    n, w, h = 400, 64, 64
    u = camera_u(w, h)
    pos, scl, rot, col = ER.make_cloud(n, 31, 0.5, 0.08, degenerate=False)
    t = lambda a: torch.tensor(np.ascontiguousarray(a, np.float32), device="cuda")  # noqa: E731
    gt_pos, gt_ls, gt_rot = t(pos[:, :3]), torch.log(t(scl[:, :2])), t(rot)
    gt_ol, gt_cl = torch.logit(t(col[:, 3]).clamp(0.05, 0.95)), torch.logit(t(col[:, :3]).clamp(0.05, 0.95))

    def frame(p, ls, q, ol, cl):
        rgb, alpha, depth = AG.render_surfels(u, p, torch.exp(ls), q, torch.sigmoid(ol), colors=torch.sigmoid(cl), width=w, height=h,
                                              return_depth=True)
        return rgb, torch.where(alpha > 0, depth, torch.zeros_like(depth)) * alpha  # (the accumulated depth: finite everywhere)
    with torch.no_grad():
        target, target_d = (a.clone() for a in frame(gt_pos, gt_ls, gt_rot, gt_ol, gt_cl))
    g = torch.Generator(device="cuda").manual_seed(5)
    params = [(gt_pos + 0.01 * torch.randn(gt_pos.shape, device="cuda", generator=g)).requires_grad_(),
              (gt_ls + 0.2 * torch.randn(gt_ls.shape, device="cuda", generator=g)).requires_grad_(),
              (gt_rot + 0.2 * torch.randn(gt_rot.shape, device="cuda", generator=g)).requires_grad_(),
              (gt_ol + 1.0 * torch.randn(gt_ol.shape, device="cuda", generator=g)).requires_grad_(),
              (gt_cl + 1.0 * torch.randn(gt_cl.shape, device="cuda", generator=g)).requires_grad_()]
    opt = torch.optim.Adam([{"params": [params[0]], "lr": 1e-3}, {"params": params[1:3], "lr": 3e-2}, {"params": params[3:], "lr": 1e-1}])
    t0 = time.time()
    losses = []
    for _ in range(60):
        opt.zero_grad()
        rgb, dacc = frame(*params)
        loss = ((rgb - target) ** 2).mean() + 0.1 * ((dacc - target_d) ** 2).mean()
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    print(f"surfel fitting: loss {losses[0]:.4g} -> {losses[-1]:.4g} ({losses[0] / losses[-1]:.1f}x) in {time.time() - t0:.1f} s")
    assert all(np.isfinite(losses)) and all(torch.isfinite(p).all() for p in params)
    assert losses[-1] <= losses[0] / 10
