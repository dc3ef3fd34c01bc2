"""Feature channels of a frame through the raw C ABI (include/splat.h, "Feature channels of a frame":
splat_composite_features, splat_composite_features_backward), against tests/features_ref.py on the four scenes of
tests/composite_grad_terms_ref.py under both forward update orders, K in {1, 3, 4, 5, 8, 9, 32} (widths 1, 3, 4, 6, 8, 12, 32 of
the kernels).

Forward: every unmasked pixel and channel within 4 c_fwd m_px[k], m_px[k] = sum w |f[k]| in float64, c_fwd the largest
|F32 - F64| / m_px of the binary32 restatement of the kernel's own formulas (never the kernel) on the same scene, order and K.
Backward: every reached splat and each of the 6 + K numbers within 4 c_scene m[s, k]; relative L2 per number at most 8 times the
restatement's.  The 4 is the project's margin over its restatement for what NumPy cannot mirror: v_exp_f32's ulp, contraction,
the summation order.  Against the kernels that exist: K = 1, f = 1 is the alpha AOV within 2 (L_px + 1) 2^-24 (each step rounds
w, T and the running sum once, each by at most 2^-25 absolute); K = 3, f = rgb gives splat_composite_backward's rgb columns
within 2 c_scene m (the same sums in another arrival order) and the image minus (1 - alpha) bg within 4 c_fwd m_px + 2^-22.

Measured on one MI355X ("Feature channels of a frame"), the worst over K of the kernel's err / c m per scene, the same
under both update orders to the digits shown unless two are given (quadrant / px):
               forward err / (c_fwd m_px)   backward err / (c_scene m)   backward relative L2 / the restatement's
    hazy       0.69                         1.16 / 1.18                  1.07 / 1.13
    veil       0.80                         1.47 / 1.27                  1.40 / 1.42
    needle     0.85                         0.88 / 1.39                  1.13 / 1.07
    classic    0.66                         3.76 / 3.69                  5.36 / 4.57
The largest forward ratio is 0.85 (needle, K = 32: 156.0 against c_fwd = 182.6, in units of 2^-24); the largest backward ratio
3.76 (classic, quadrant, K = 32: splat 2453, B00, 184.2 against c_scene = 49.0 x 2^-24), the largest L2 ratio 5.36 (classic,
quadrant, K = 1).  classic's constant is a maximum over 3000 splats of a heavy-tailed figure (44.7 to 297.5 x 2^-24 over the
seven K): dA = T (s - S) cancels where s is close to S, and the rounding of the K-term dot s scales with sum |G f|, not with
|s - S|; the kernel and the restatement round that dot differently (contraction), so each has its own worst splat.
|F - alpha| for f = 1: at most 27 x 2^-24 (veil), never closer than 2 x 2^-24 to its bound.  grad_features against
splat_composite_backward's rgb columns: at most 0.03 c_scene.  Autograd against the ABI: 0.01 c_scene.
"""
import ctypes as C

import numpy as np
import pytest

from splat_renderer_amd import _lib
from tests import composite_grad_terms_ref as CT
from tests import ellipsoid_grad_ref as GR
from tests import ellipsoid_ref as ER
from tests import features_ref as FR
from tests import test_gpu_ellipsoid_grad as TG
from tests import test_gpu_grad_decisions as TDEC

pytestmark = pytest.mark.gpu

KERNEL = {"quadrant": 0, "px": 1}  # splat_composite_options' forward kernel: k_composite, k_composite_px
CHANNELS = (1, 3, 4, 5, 8, 9, 32)
MARGIN, DET_MARGIN, L2_MARGIN = 4.0, 2.0, 8.0
SENT = np.float32(7.0)
WIDE, WIDE_COL0 = 40, 2  # the strided layout: columns [2, 2 + K) of an (n, 40) buffer whose base is 4 bytes into its allocation
GUARD = 64               # floats past the end of `out` that must keep the sentinel
INVALID = -1


class Frame:
    """A scene's records, colours and lists on the device."""

    def __init__(self, d, rec, col, counts, offsets, idx, w, h):
        self.d, self.w, self.h, self.n = d, w, h, rec.shape[0]
        self.bufs = [d.createBufferFrom(np.ascontiguousarray(a)) for a in (rec, col, idx if idx.size else np.zeros(1, np.uint32), counts, offsets)]

    def args(self, cfg=None):
        b = self.bufs
        return (self.d.ctx, C.byref(cfg or TG.cfg()), b[1].ptr, 1, b[0].ptr, b[2].ptr, b[3].ptr, b[4].ptr, self.w, self.h)

    def destroy(self):
        for b in self.bufs:
            b.destroy()


def scene_frame(d, name):
    s = CT.scene(name)
    return Frame(d, s["rec"], s["col"], s["counts"], s["offsets"], s["idx"], s["w"], s["h"])


def rows_buffer(d, a, wide, fill=SENT):
    """(buffer, pointer, stride, host image) of (n, K) rows on the device: packed, or (wide) as columns [2, 2 + K) of an (n, 40)
    buffer, the other columns `fill`, whose base is 4 bytes into its allocation."""
    n, K = a.shape
    if not wide:
        b = d.createBufferFrom(a)
        return b, b.ptr, K, np.ascontiguousarray(a, np.float32)
    host = np.full((n, WIDE), fill, np.float32)
    host[:, WIDE_COL0:WIDE_COL0 + K] = a
    b = d.createBuffer(4 + host.nbytes + 12)
    b.write(host, 4)
    return b, b.ptr + 4 + 4 * WIDE_COL0, WIDE, host


def forward(d, fr, f, wide=False, n=None, cfg=None, channels=None, stride=None, fptr_shift=0, null_out=False):
    """(rc, out (H W, K) float32, the GUARD floats behind it) of one splat_composite_features call; out is filled with the
    sentinel first."""
    K = f.shape[1]
    fb, fptr, fstride, _ = rows_buffer(d, f, wide)
    npx = fr.w * fr.h
    out = d.createBufferFrom(np.full(npx * K + GUARD, SENT, np.float32))
    rc = d.lib.splat_composite_features(*fr.args(cfg), fptr + fptr_shift, fstride if stride is None else stride, K if channels is None else channels,
                                        fr.n if n is None else n, None if null_out else out.ptr)
    d.sync()
    got = out.read(np.float32)
    for b in (fb, out):
        b.destroy()
    return rc, got[:npx * K].reshape(npx, K), got[npx * K:]


def backward(d, fr, f, gf, wide=False, n=None, cfg=None, channels=None, stride=None, gstride=None, fptr_shift=0, null_gout=False, fill=0.0):
    """(rc, grad_records (n, 8), grad_color_opacity (n, 4), grad_features (n, K), the wide gradient buffer's host image or None)
    of one splat_composite_features_backward call.  The cells the call adds into start at `fill`, every other cell (records
    columns 4, 6, 7, colour columns 0 - 2, the other columns of a wide feature buffer) at the sentinel."""
    K = f.shape[1]
    fb, fptr, fstride, _ = rows_buffer(d, f, wide)
    gout = d.createBufferFrom(np.ascontiguousarray(gf, np.float32).reshape(-1))
    grec0 = np.full((fr.n, 8), fill, np.float32)
    grec0[:, [4, 6, 7]] = SENT
    gcol0 = np.full((fr.n, 4), SENT, np.float32)
    gcol0[:, 3] = fill
    grec, gcol = d.createBufferFrom(grec0), d.createBufferFrom(gcol0)
    gb, gptr, gs, _ = rows_buffer(d, np.full((fr.n, K), fill, np.float32), wide)
    rc = d.lib.splat_composite_features_backward(*fr.args(cfg), fptr + fptr_shift, fstride if stride is None else stride,
                                                 K if channels is None else channels, None if null_gout else gout.ptr, fr.n if n is None else n,
                                                 grec.ptr, gcol.ptr, gptr, gs if gstride is None else gstride)
    d.sync()
    r, c = grec.read(np.float32, fr.n * 8).reshape(fr.n, 8), gcol.read(np.float32, fr.n * 4).reshape(fr.n, 4)
    if wide:
        whole = gb.read(np.float32, fr.n * WIDE, offset=4).reshape(fr.n, WIDE)
        gfeat = whole[:, WIDE_COL0:WIDE_COL0 + K].copy()
    else:
        whole, gfeat = None, gb.read(np.float32, fr.n * K).reshape(fr.n, K)
    for b in (fb, gout, grec, gcol, gb):
        b.destroy()
    return rc, r, c, gfeat, whole


def numbers(grec, gcol, gfeat):
    """(n, 6 + K) in features_ref's column order."""
    return np.concatenate([grec[:, CT.REC_COLS], gcol[:, 3:4], gfeat], axis=1)


_frames = {}


@pytest.fixture
def frames(device):
    """name -> Frame of a scene, uploaded once per session's device."""
    def get(name):
        key = (id(device), name)
        if key not in _frames:
            _frames[key] = scene_frame(device, name)
        return _frames[key]
    return get


class forced:
    """with forced(device, order): the forward update order forced on the context, the default restored after."""

    def __init__(self, d, order):
        self.d, self.order = d, order

    def __enter__(self):
        TDEC.with_kernel(self.d, KERNEL[self.order])

    def __exit__(self, *exc):
        TDEC.with_kernel(self.d, -1)


# ---- against the reference ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", CHANNELS)
@pytest.mark.parametrize("order", FR.ORDERS)
@pytest.mark.parametrize("name", FR.SCENES)
def test_forward_against_the_reference(device, frames, name, order, K):
    f, _ = FR.inputs(name, K)
    t64, ref = FR.terms64(name, K), FR.restated(name, order, K)
    with forced(device, order):
        rc, got, tail = forward(device, frames(name), f)
    assert rc == 0 and np.isfinite(got).all() and (tail == SENT).all()
    ok = ~FR.masked(name).reshape(-1)
    q = CT.ratios(got, t64["F"], t64["m_px"])[ok]
    print(f"{name} {order} K={K}: kernel worst err / m_px = {q.max() * 2 ** 24:.1f} x 2^-24 against c_fwd = {ref['c_fwd'] * 2 ** 24:.1f} x 2^-24: "
          f"ratio {q.max() / ref['c_fwd']:.2f}")
    # a pixel whose tile list is empty, or that consumed nothing: exact 0
    empty = ok & (t64["L_px"] == 0)
    assert empty.any() and (got[empty] == 0).all()
    assert (q <= MARGIN * ref["c_fwd"]).all(), f"{int((q > MARGIN * ref['c_fwd']).sum())} (pixel, channel) values beyond {MARGIN:g} c_fwd m_px"


@pytest.mark.parametrize("K", CHANNELS)
@pytest.mark.parametrize("order", FR.ORDERS)
@pytest.mark.parametrize("name", FR.SCENES)
def test_backward_against_the_reference(device, frames, name, order, K):
    s = CT.scene(name)
    f, gf = FR.inputs(name, K)
    t64, ref = FR.terms64(name, K), FR.restated(name, order, K)
    with forced(device, order):
        rc, grec, gcol, gfeat, _ = backward(device, frames(name), f, gf)
    assert rc == 0
    got, want, m = numbers(grec, gcol, gfeat), t64["sum"], t64["m"]
    assert got.shape == want.shape and np.isfinite(got).all()
    # untouched cells keep the sentinel; splats no consumed pair reaches are exact zeros
    assert (grec[:, [4, 6, 7]] == SENT).all() and (gcol[:, :3] == SENT).all()
    assert (got[~s["reached"]] == 0).all()
    q = CT.ratios(got, want, m)
    worst = np.unravel_index(np.argmax(q), q.shape)
    l2 = np.array([CT.rel_l2(got[:, k], want[:, k]) for k in range(want.shape[1])])
    print(f"{name} {order} K={K}: kernel worst err / m = {q.max() * 2 ** 24:.1f} x 2^-24 (splat {worst[0]}, {FR.names(K)[worst[1]]}) against c_scene = "
          f"{ref['c_scene'] * 2 ** 24:.1f} x 2^-24: ratio {q.max() / ref['c_scene']:.2f}; relative L2 worst ratio to the restatement's "
          f"{np.max(l2 / ref['l2']):.2f}")
    bad = q[s["reached"]] > MARGIN * ref["c_scene"]
    assert not bad.any(), f"{int(bad.sum())} (splat, number) sums beyond {MARGIN:g} c_scene m; the worst {q.max() / ref['c_scene']:.2f} c_scene"
    for k in range(want.shape[1]):
        assert l2[k] <= L2_MARGIN * ref["l2"][k], f"{FR.names(K)[k]}: relative L2 {l2[k]:.3g} against the restatement's {ref['l2'][k]:.3g}"


# ---- strides and edges --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [1, 5, 32])
def test_strided_rows_give_the_packed_bits(device, frames, K):
    name = "veil"
    f, gf = FR.inputs(name, K)
    fr = frames(name)
    rc0, out0, tail0 = forward(device, fr, f)
    rc1, out1, tail1 = forward(device, fr, f, wide=True)
    assert rc0 == 0 and rc1 == 0 and (tail0 == SENT).all() and (tail1 == SENT).all()
    assert np.array_equal(out0.view(np.uint32), out1.view(np.uint32))
    assert np.abs(out0).max() > 0.1
    rc0, grec0, gcol0, gfeat0, _ = backward(device, fr, f, gf)
    rc1, grec1, gcol1, gfeat1, whole = backward(device, fr, f, gf, wide=True)
    assert rc0 == 0 and rc1 == 0
    # the other columns of the wide gradient buffer keep their sentinel
    other = np.ones(WIDE, bool)
    other[WIDE_COL0:WIDE_COL0 + K] = False
    assert (whole[:, other] == SENT).all()
    # the same sums in another arrival order
    s, ref, t64 = CT.scene(name), FR.restated(name, "quadrant", K), FR.terms64(name, K)
    q = CT.ratios(numbers(grec1, gcol1, gfeat1), numbers(grec0, gcol0, gfeat0).astype(np.float64), t64["m"])
    assert (q <= DET_MARGIN * ref["c_scene"]).all() and np.abs(gfeat1[s["reached"]]).max() > 0


def one_tile_cloud():
    """65 splats of low opacity that all bin into the one tile of a 16 x 16 screen."""
    pos, scl, rot, col = ER.make_cloud(100, 3, 0.15, 0.2)
    u = TG.camera_u(16, 16)
    _, _, _, idx = TG.lists(u, pos, scl, rot, 16, 16)
    keep = np.sort(idx)[:65]
    assert keep.shape[0] == 65
    col = col[keep].copy()
    col[:, 3] = 0.02
    return u, pos[keep], scl[keep], rot[keep], col


@pytest.mark.parametrize("n", [1, 63, 64, 65])
def test_list_lengths_around_a_chunk(device, n):
    """The first n of 65 splats in one tile: lists of 1, 63, 64 and 65 entries (one chunk is 64).  `out` is the same bits
    whether the buffers hold n rows or all 65 (the rows from n on NaN) and whether the call's n is n or 65: n sizes nothing."""
    u, pos, scl, rot, col = one_tile_cloud()
    K = 3
    f = np.random.default_rng(n).uniform(-2, 2, (65, K)).astype(np.float32)
    rec, counts, offsets, idx = TG.lists(u, pos[:n], scl[:n], rot[:n], 16, 16)
    assert counts.tolist() == [n]
    small = Frame(device, rec, col[:n], counts, offsets, idx, 16, 16)
    rec_all = np.concatenate([rec, np.full((65 - n, 8), np.nan, np.float32)])
    f_all = f.copy()
    f_all[n:] = np.nan
    big = Frame(device, rec_all, col, counts, offsets, idx, 16, 16)
    outs = [forward(device, small, f[:n]), forward(device, big, f_all, n=n), forward(device, big, f_all)]
    for fr in (small, big):
        fr.destroy()
    for rc, out, tail in outs:
        assert rc == 0 and np.isfinite(out).all() and (tail == SENT).all()
        assert np.array_equal(out.view(np.uint32), outs[0][1].view(np.uint32))
    # float64 over the same pairs: within the forward bound's form with the hazy scenes' order of constant (64 x 2^-24)
    dec = GR.decisions(rec, col[:n], idx, counts, offsets, 16, 16)
    import torch
    with torch.no_grad():
        t = lambda a: torch.tensor(np.asarray(a, np.float64))  # noqa: E731
        want = FR.features64(t(rec), t(col[:n]), t(f[:n]), dec["steps"], 16, 16).numpy()
        m_px = FR.features64(t(rec), t(col[:n]), t(np.abs(f[:n])), dec["steps"], 16, 16).numpy()
    ok = ~(dec["rim"] | dec["near"]).reshape(-1)
    assert (np.abs(outs[0][1] - want)[ok] <= 64 * 2.0 ** -24 * m_px[ok]).all() and m_px.max() > 0


def test_no_splats(device, frames):
    fr = frames("hazy")
    K = 4
    f, gf = FR.inputs("hazy", K)
    rc, out, tail = forward(device, fr, f, n=0)
    assert rc == 0 and (out == 0).all() and (tail == SENT).all()
    rc, grec, gcol, gfeat, _ = backward(device, fr, f, gf, n=0, fill=SENT)
    assert rc == 0 and (grec == SENT).all() and (gcol == SENT).all() and (gfeat == SENT).all()


# ---- against the kernels that exist -------------------------------------------------------------------------------------------
def drawn(device, name):
    """(image (H W, 4), alpha (H W,)) of splat_composite_aov on a scene, under the context's current forward kernel."""
    s = CT.scene(name)
    fr = TDEC.Frame(device, s["rec"], s["col"], s["counts"], s["offsets"], s["idx"], s["w"], s["h"])
    img, alpha = fr.forward(want_alpha=True)
    fr.destroy()
    return img.reshape(-1, 4), alpha.reshape(-1)


@pytest.mark.parametrize("order", FR.ORDERS)
@pytest.mark.parametrize("name", FR.SCENES)
def test_a_feature_of_one_is_the_alpha_aov(device, frames, name, order):
    s = CT.scene(name)
    with forced(device, order):
        rc, got, _ = forward(device, frames(name), np.ones((s["n"], 1), np.float32))
        _, alpha = drawn(device, name)
    assert rc == 0
    L = FR.terms64(name, 1)["L_px"]
    err = np.abs(got[:, 0].astype(np.float64) - alpha)
    print(f"{name} {order}: |F - alpha| at most {err.max() * 2 ** 24:.1f} x 2^-24; the bound's smallest slack {np.min(2 * (L + 1) - err * 2 ** 24):.1f} x 2^-24")
    assert (err <= 2 * (L + 1) * 2.0 ** -24).all()
    assert alpha.max() > 0.5


@pytest.mark.parametrize("order", FR.ORDERS)
@pytest.mark.parametrize("name", FR.SCENES)
def test_rgb_as_features_is_the_image(device, frames, name, order):
    s = CT.scene(name)
    f = np.ascontiguousarray(s["col"][:, :3])
    ref = FR.restated(name, order, 3)
    _, m_px = FR.forward64(name, f)
    with forced(device, order):
        rc, got, _ = forward(device, frames(name), f)
        img, alpha = drawn(device, name)
    assert rc == 0
    want = img[:, :3].astype(np.float64) - (1.0 - alpha.astype(np.float64))[:, None] * np.array(GR.BG, np.float32).astype(np.float64)[None, :]
    # m_px = sum w |f| = sum w f = F for colours >= 0: at masked pixels, where the reference's decisions are not the kernels',
    # the kernel's own F stands in for it
    msk = FR.masked(name).reshape(-1)
    m_use = np.where(msk[:, None], got.astype(np.float64), m_px)
    assert (f >= 0).all()
    err = np.abs(got - want)
    assert (err <= MARGIN * ref["c_fwd"] * m_use + 2.0 ** -22).all(), f"worst excess {np.max(err - MARGIN * ref['c_fwd'] * m_use) * 2 ** 24:.1f} x 2^-24"


@pytest.mark.parametrize("order", FR.ORDERS)
@pytest.mark.parametrize("name", FR.SCENES)
def test_rgb_feature_gradient_is_the_colour_gradient(device, frames, name, order):
    """K = 3, f = rgb, G_F = the image's G_rgb, G_A = 0: grad_features is splat_composite_backward's rgb columns, the same sums in
    another arrival order."""
    s = CT.scene(name)
    f = np.ascontiguousarray(s["col"][:, :3])
    g = s["g"].copy()
    g[..., 3] = 0
    c = CT.restated(name, order, False)["c"]
    with forced(device, order):
        rc, _, _, gfeat, _ = backward(device, frames(name), f, np.ascontiguousarray(g[..., :3]))
        rc2, _, gcol = TG.composite_backward(device, s["rec"], s["col"], s["counts"], s["offsets"], s["idx"], s["w"], s["h"], g)
    assert rc == 0 and rc2 == 0
    q = CT.ratios(gfeat, gcol[:, :3].astype(np.float64), s["m"][:, 5:8])
    print(f"{name} {order}: |grad_features - grad rgb| / m at most {q.max() * 2 ** 24:.1f} x 2^-24 = {q.max() / c:.2f} c_scene")
    assert (q <= DET_MARGIN * c).all() and np.abs(gfeat).max() > 0


# ---- rejections ---------------------------------------------------------------------------------------------------------------
REJECTIONS = {
    "channels 0": dict(channels=0),
    "channels 33": dict(channels=33, stride=64),
    "stride below channels": dict(stride=3),
    "misaligned features": dict(fptr_shift=2),
    "strict band": dict(cfg=dict(tile_row0=1)),
}


@pytest.mark.parametrize("case", list(REJECTIONS) + ["null out"])
def test_forward_rejections(device, frames, case):
    f, _ = FR.inputs("hazy", 4)
    kw = dict(REJECTIONS.get(case, dict(null_out=True)))
    if "cfg" in kw:
        kw["cfg"] = TG.cfg(**kw["cfg"])
    rc, out, tail = forward(device, frames("hazy"), f, **kw)
    assert rc == INVALID and (out == SENT).all() and (tail == SENT).all()


@pytest.mark.parametrize("case", list(REJECTIONS) + ["null grad_out", "grad stride below channels"])
def test_backward_rejections(device, frames, case):
    f, gf = FR.inputs("hazy", 4)
    kw = dict(REJECTIONS.get(case, dict(null_gout=True) if case == "null grad_out" else dict(gstride=3)))
    if "cfg" in kw:
        kw["cfg"] = TG.cfg(**kw["cfg"])
    rc, grec, gcol, gfeat, _ = backward(device, frames("hazy"), f, gf, fill=SENT, **kw)
    assert rc == INVALID and (grec == SENT).all() and (gcol == SENT).all() and (gfeat == SENT).all()
