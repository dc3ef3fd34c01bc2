"""The Gaussian gradients splat by splat, on the clouds where a sum can go wrong unseen: hazy (a pixel consumes hundreds of
pairs), veil (pixels stop deep in their lists, off the chunk boundaries), needle (cond(Sigma2) up to 1.6e4) and the other
gradient tests' first case (tests/composite_grad_terms_ref.py builds them; tests/test_composite_grad_terms_cpu.py holds them to
their purpose).

Composite backward (splat_composite_backward, _depth, _det with and without depth, under both forward update orders): for every
reached splat s and every number k
    |got - autograd| <= 4 c_scene m[s, k]
m[s, k] = the sum over the splat's pairs of |term| in float64, c_scene = the largest |sum32 - autograd| / m of the plain
binary32 restatement of the kernel's own formulas on the same scene, order and depth variant (terms32: never the kernel).  The 4
covers what the restatement cannot mirror: the kernel's addition order (DPP tree, four waves, atomics or the fixed-order gather)
against a sequential sum, v_exp_f32's 1 ulp against NumPy's half ulp, and contraction.  Unreached splats and the columns nobody
writes are exact zeros.  Per number the relative L2 is at most 8 times terms32's own.  On hazy and veil the fixed-order result
lies within 2 c_scene m of the atomic one: the same sums in another order.

Projector backward (splat_project_ellipsoid_backward, _depth, _aa and the per-splat outputs of _camera), on the needle and the
classic clouds under the default camera and tests/cameras.py's orbit_off_target, every unculled splat, no conditioning
exclusion: for every component of position, scale and rotation
    |got - want| <= 2^-23 |want| + 64 cond_s 2^-52 max_k |want_s|
want = float64 autograd over records64 (and depth64, rho64), cond_s = cond(Sigma2), max_k over the splat's ten components.  The
first term is the kernel's single rounding to binary32 (and the reference's own float64 error); the second the cancellation in
det = A C - B^2 in float64: some 64 operations feed it and follow it, each off by 2^-53 relative, amplified by cond.

Measured on one MI355X ("Gradients of the ellipsoid footprint", "Per-splat bounds"), the kernel's worst err / m against
c_scene, both in units of 2^-24, the same for the atomic and the fixed-order entry points to the digit shown:
             quadrant colour   quadrant depth    px colour         px depth
    hazy      10.6 /  10.6      26.8 /  26.7      8.6 /  10.6      23.2 /  21.1
    veil      21.1 /  23.4      21.3 /  22.4     20.2 /  23.1      19.5 /  24.0
    needle    18.1 /  25.9      18.2 /  29.5     20.4 /  27.8      15.1 /  29.5
    classic  109.5 /  62.8     174.7 /  95.0    109.5 /  62.8      36.7 /  95.0
The largest ratio is 1.84 (classic, quadrant, depth); relative L2 per number 0.78 to 2.41 times terms32's; |det - atomic| / m at
most 1.0 x 2^-24 (0.09 c_scene).  Projector: the worst err / bound is 0.497 in all sixteen cases (cond up to 1.35e5): the single
rounding to binary32, the cond term never needed.
"""
import functools

import numpy as np
import pytest
import torch

from tests import cameras as CAMS
from tests import composite_grad_terms_ref as CT
from tests import ellipsoid_aa_ref as AR
from tests import ellipsoid_depth_grad_ref as DR
from tests import ellipsoid_grad_ref as GR
from tests import test_gpu_ellipsoid_aa as TA
from tests import test_gpu_ellipsoid_depth_grad as TD
from tests import test_gpu_ellipsoid_grad as TG
from tests import test_gpu_grad_decisions as TDEC
from tests import test_gpu_grad_deterministic as TDET

pytestmark = pytest.mark.gpu

KERNEL = {"quadrant": 0, "px": 1}  # splat_composite_options' forward kernel: k_composite, k_composite_px
ENTRIES = ("atomic", "atomic_depth", "det", "det_depth")
MARGIN = 4.0
DET_MARGIN = 2.0
L2_MARGIN = 8.0

_results = {}


def run_entry(device, name, order, entry):
    """(n, 9 | 10) float32 in terms' column order, and the raw grad_records: one call of one entry point on a scene with the
    forward update order forced.  Each combination runs once per session."""
    key = (name, order, entry)
    if key in _results:
        return _results[key]
    s = CT.scene(name)
    depth = entry.endswith("depth")
    TDEC.with_kernel(device, KERNEL[order])
    try:
        if entry.startswith("det"):
            run = TDET.Det(device, s)
            rc, grec, gcol, gz = run.run(s["g"], s["gd"] if depth else None)
            run.destroy()
        elif depth:
            rc, grec, gcol, gz = TD.composite_backward_depth(device, s["rec"], s["col"], s["z"], s["counts"], s["offsets"], s["idx"], s["w"], s["h"],
                                                             s["g"], s["gd"])
        else:
            rc, grec, gcol = TG.composite_backward(device, s["rec"], s["col"], s["counts"], s["offsets"], s["idx"], s["w"], s["h"], s["g"])
            gz = None
    finally:
        TDEC.with_kernel(device, -1)
    assert rc == 0
    cols = [grec[:, CT.REC_COLS], gcol] + ([gz[:, None]] if depth else [])
    _results[key] = (np.concatenate(cols, axis=1), grec)
    return _results[key]


@pytest.mark.parametrize("entry", ENTRIES)
@pytest.mark.parametrize("order", CT.ORDERS)
@pytest.mark.parametrize("name", CT.SCENES)
def test_composite_backward_per_splat(device, name, order, entry):
    s = CT.scene(name)
    depth = entry.endswith("depth")
    ref = CT.restated(name, order, depth)
    want, m = (s["want_depth"], s["m_depth"]) if depth else (s["want"], s["m"])
    got, grec = run_entry(device, name, order, entry)
    assert got.shape == want.shape and np.isfinite(got).all()
    q = CT.ratios(got, want, m)
    worst = np.unravel_index(np.argmax(q), q.shape)
    l2 = np.array([CT.rel_l2(got[:, k], want[:, k]) for k in range(want.shape[1])])
    print(f"{name} {order} {entry}: kernel worst err / m = {q.max() * 2 ** 24:.1f} x 2^-24 (splat {worst[0]}, {CT.NAMES[worst[1]]}) against "
          f"c_scene = {ref['c'] * 2 ** 24:.1f} x 2^-24: ratio {q.max() / ref['c']:.2f}; relative L2 at most {l2.max():.3g} against "
          f"terms32's {ref['l2'].max():.3g}: worst ratio {np.max(l2 / ref['l2']):.2f}")
    # splats no consumed pair reaches, and the columns nobody writes: exact zeros
    assert (got[~s["reached"]] == 0).all()
    assert (grec[:, [4, 6, 7]] == 0).all()
    bad = q > MARGIN * ref["c"]
    assert not bad.any(), (f"{int(bad.sum())} (splat, number) sums beyond {MARGIN:g} c_scene m; the worst at splat {worst[0]}, {CT.NAMES[worst[1]]}: "
                           f"err / m = {q.max() * 2 ** 24:.1f} x 2^-24 = {q.max() / ref['c']:.2f} c_scene")
    for k in range(want.shape[1]):
        assert l2[k] <= L2_MARGIN * ref["l2"][k], f"{CT.NAMES[k]}: relative L2 {l2[k]:.3g} against terms32's {ref['l2'][k]:.3g}"


@pytest.mark.parametrize("depth", [False, True], ids=["colour", "depth"])
@pytest.mark.parametrize("order", CT.ORDERS)
@pytest.mark.parametrize("name", ["hazy", "veil"])
def test_fixed_order_sums_are_the_atomic_sums(device, name, order, depth):
    s = CT.scene(name)
    ref = CT.restated(name, order, depth)
    m = s["m_depth"] if depth else s["m"]
    a, _ = run_entry(device, name, order, "atomic_depth" if depth else "atomic")
    d, _ = run_entry(device, name, order, "det_depth" if depth else "det")
    q = CT.ratios(d, a.astype(np.float64), m)
    print(f"{name} {order} {'depth' if depth else 'colour'}: |det - atomic| / m at most {q.max() * 2 ** 24:.1f} x 2^-24 = {q.max() / ref['c']:.2f} c_scene")
    assert (q <= DET_MARGIN * ref["c"]).all()


# ---- the projector ---------------------------------------------------------------------------------------------------------
CLOUDS = ("needle", "classic")
CAMERAS = ("orbit_default", "orbit_off_target")
PROJ_ENTRIES = ("plain", "depth", "aa", "camera")


@functools.lru_cache(maxsize=None)
def projector_case(cloud, camera):
    """A cloud under a camera: upstreams, culls, cond(Sigma2), the binary32 rho and the float64 gradients of the four losses."""
    pos, scl, rot, _col, w, h, seed = CT.make_scene_cloud(cloud)
    n = pos.shape[0]
    u = CAMS.camera(camera, w, h)
    rng = np.random.default_rng(seed + 50)
    grec = rng.uniform(-1, 1, (n, 8)).astype(np.float32)
    gz = rng.uniform(-1, 1, n).astype(np.float32)
    grho = rng.uniform(-1, 1, n).astype(np.float32)
    cull = GR.culled(u, pos, scl, rot)
    cond = GR.sigma2_cond(u, pos, scl, rot)
    rho = AR.rho32(u, pos, scl, rot)
    t = lambda a: torch.tensor(np.asarray(a, np.float64))  # noqa: E731
    # where rho is differentiated: the binary32 rho positive and the float64 det0 positive (elsewhere the term is exactly zero)
    with torch.no_grad():
        r64 = AR.rho64(u, t(pos), t(scl), t(rot), ~cull & (rho > 0)).numpy()
    live = ~cull & (rho > 0) & np.isfinite(r64) & (r64 > 0)
    rows = torch.as_tensor(np.nonzero(~cull)[0], dtype=torch.long)
    want = {}
    for which in ("plain", "depth", "aa"):
        P, S, Q = (torch.tensor(a.astype(np.float64), requires_grad=True) for a in (pos, scl, rot))
        L = (GR.records64(u, P, S, Q, ~cull) * t(grec)).sum()
        if which == "depth":
            L = L + (DR.depth64(u, P[rows]) * t(gz)[rows]).sum()
        if which == "aa":
            L = L + (AR.rho64(u, P, S, Q, live) * t(grho)).sum()
        L.backward()
        want[which] = np.concatenate([P.grad.numpy()[:, :3], S.grad.numpy()[:, :3], Q.grad.numpy()], axis=1)
    want["camera"] = want["depth"]
    out = dict(pos=pos, scl=scl, rot=rot, u=u, n=n, grec=grec, gz=gz, grho=grho, cull=cull, cond=cond, rho=rho, live=live, want=want)
    for v in list(out.values()) + list(want.values()):
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


@pytest.mark.parametrize("which", PROJ_ENTRIES)
@pytest.mark.parametrize("camera", CAMERAS)
@pytest.mark.parametrize("cloud", CLOUDS)
def test_project_backward_per_splat(device, cloud, camera, which):
    c = projector_case(cloud, camera)
    cull, cond, want = c["cull"], c["cond"], c["want"][which]
    kept = ~cull
    assert kept.sum() >= c["n"] // 2
    if (cloud, camera) == ("needle", "orbit_default"):
        assert (cond[kept] > 1e4).sum() >= 10
    if which == "aa":
        assert c["live"].sum() >= kept.sum() // 2
    depth = which in ("depth", "camera")
    rc, gp, gs, gq, _ = TA.backward_aa(device, c["u"], c["pos"], c["scl"], c["rot"], c["grec"], c["gz"] if depth else None, c["grho"], cam=False,
                                       which=which)
    assert rc == 0
    assert (gp[:, 3] == 0).all() and (gs[:, 3] == 0).all()
    got = np.concatenate([gp[:, :3], gs[:, :3], gq], axis=1)
    assert np.isfinite(got).all() and (got[cull] == 0).all()
    top = np.abs(want[kept]).max(axis=1, keepdims=True)
    bound = 2.0 ** -23 * np.abs(want[kept]) + 64.0 * cond[kept, None] * 2.0 ** -52 * top
    err = np.abs(got[kept].astype(np.float64) - want[kept])
    with np.errstate(all="ignore"):
        ratio = np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err > 0, np.inf, 0.0))
    worst = np.unravel_index(np.argmax(ratio), ratio.shape)
    print(f"{cloud} {camera} {which}: worst err / bound {ratio.max():.3f} (splat {np.nonzero(kept)[0][worst[0]]}, component {worst[1]}, cond "
          f"{cond[kept][worst[0]]:.3g}); largest cond {cond[kept].max():.3g}")
    assert (err <= bound).all(), f"{int((err > bound).sum())} components beyond the bound, the worst {ratio.max():.3g} times"
    if which == "aa":
        # no rho term where the binary32 rho is 0 or the float64 det0 is not positive: the classic backward's bits
        off = kept & ~c["live"]
        _, cp, cs, cq, _ = TA.backward_aa(device, c["u"], c["pos"], c["scl"], c["rot"], c["grec"], None, c["grho"], which="plain")
        for a, b in ((gp, cp), (gs, cs), (gq, cq)):
            assert np.array_equal(TA.bits(a[off]), TA.bits(b[off]))
