"""The ABI promises of the backward entry points (include/splat.h) that the float64 comparisons cannot see: grad_records,
grad_color_opacity and grad_depth are ADDED into (a kernel that overwrote them fails the pre-filled buffers here); columns 4, 6
and 7 of grad_records and the SH pad floats past 3 (degree + 1)^2 keep a NaN-payload sentinel bit for bit (a stray write
fails); the w words of the overwritten n x 4 outputs are 0; and every stride argument is honoured (a kernel that ignored one
reads other splats' words: the results would differ from the packed call's)."""
import ctypes as C

import numpy as np
import pytest

from tests import ellipsoid_ref as ER
from tests import test_gpu_ellipsoid_grad as TG

pytestmark = pytest.mark.gpu
SENT = np.uint32(0x7FC0BEEF)  # a quiet NaN with a payload: no kernel arithmetic produces these bits


def _f(a):
    return np.ascontiguousarray(a, np.float32)


def _run_composite(d, rec, col, cstride, counts, offsets, idx, w, h, g, gd, z, zstride, pre_rec, pre_col, pre_z, depth=True):
    n = rec.shape[0]
    colbuf = np.zeros((n * cstride, 4), np.float32)
    colbuf[::cstride] = col
    lists = [np.ascontiguousarray(a, np.uint32) for a in (idx if idx.size else np.zeros(1, np.uint32), counts, offsets)]
    bufs = [d.createBufferFrom(a) for a in [_f(rec), _f(colbuf)] + lists + [_f(g), _f(z), _f(gd)]]
    outs = [d.createBufferFrom(a) for a in (pre_rec, pre_col, pre_z)]
    args = (d.ctx, C.byref(TG.cfg()), bufs[1].ptr, cstride, bufs[0].ptr, bufs[2].ptr, bufs[3].ptr, bufs[4].ptr, w, h, bufs[5].ptr, n,
            outs[0].ptr, outs[1].ptr)
    if depth:
        rc = d.lib.splat_composite_backward_depth(*args, bufs[6].ptr, zstride, bufs[7].ptr, outs[2].ptr)
    else:
        rc = d.lib.splat_composite_backward(*args)
    assert rc == 0
    res = [o.read(np.float32, count=a.size) for o, a in zip(outs, (pre_rec, pre_col, pre_z))]
    for b in bufs + outs:
        b.destroy()
    return res[0].reshape(n, 8), res[1].reshape(n, 4), res[2]


@pytest.mark.parametrize("depth", [False, True], ids=["colour", "depth"])
@pytest.mark.parametrize("n", [3000, 1])
def test_composite_backward_adds_and_honours_strides(device, depth, n):
    w, h = 160, 120
    pos, scl, rot, col = ER.make_cloud(n, 1, 1.0 if n > 1 else 0.0, 0.03 if n > 1 else 0.05)
    u = TG.camera_u(w, h)
    _, proj, _ = ER.project(u, pos, scl, rot)
    rec, counts, offsets, idx = TG.lists(u, pos, scl, rot, w, h)
    assert idx.size > 0
    rng = np.random.default_rng(3)
    g = rng.uniform(-1, 1, (h, w, 4)).astype(np.float32)
    gd = rng.uniform(-1, 1, (h, w)).astype(np.float32)
    z_packed = _f(proj[:, 4])
    z_rows = _f(proj.reshape(n, 8))  # the ProjectedSplat depth word: stride 8, offset 4
    zero = (np.zeros((n, 8), np.float32), np.zeros((n, 4), np.float32), np.zeros(n, np.float32))
    ref = _run_composite(device, rec, col, 1, counts, offsets, idx, w, h, g, gd, z_packed, 1, *zero, depth=depth)
    pre_rec = rng.uniform(-3, 3, (n, 8)).astype(np.float32)
    pre_rec.view(np.uint32)[:, [4, 6, 7]] = SENT
    pre_col, pre_z = rng.uniform(-3, 3, (n, 4)).astype(np.float32), rng.uniform(-3, 3, n).astype(np.float32)
    got = _run_composite(device, rec, col, 2 if depth else 3, counts, offsets, idx, w, h, g, gd, z_rows.reshape(-1)[4:], 8, pre_rec,
                         pre_col, pre_z, depth=depth)
    assert np.array_equal(got[0].view(np.uint32)[:, [4, 6, 7]], pre_rec.view(np.uint32)[:, [4, 6, 7]]), "unused columns written"
    checks = [("records", ref[0][:, TG.REC_COLS], got[0][:, TG.REC_COLS], pre_rec[:, TG.REC_COLS]), ("colour", ref[1], got[1], pre_col)]
    if depth:
        checks.append(("depth", ref[2], got[2], pre_z))
    else:
        assert np.array_equal(got[2], pre_z)  # (not an argument of the colour-only call)
    for name, r, gt, pre in checks:
        delta = gt.astype(np.float64) - pre
        # atomic-sum rounding, plus the rounding of adding into the pre-fill (|pre| <= 3)
        tol = 2e-5 * np.abs(r).max() + 4e-7 * np.abs(pre) + 1e-30
        assert (np.abs(delta - r) <= tol).all(), f"{name}: {np.abs(delta - r).max():.3g}"
        assert np.abs(r).max() > 0


def test_composite_backward_empty_lists_and_nothing_on_screen(device):
    d = device
    n, w, h = 7, 48, 40
    ntx, nty = 3, 3
    rec = np.zeros((n, 8), np.float32)  # culled records: nothing on screen
    col = np.full((n, 4), 0.5, np.float32)
    counts, offsets = np.zeros(ntx * nty, np.uint32), np.zeros(ntx * nty + 1, np.uint32)
    g = np.ones((h, w, 4), np.float32)
    pre = (np.full((n, 8), 2.0, np.float32), np.full((n, 4), -1.0, np.float32), np.full(n, 5.0, np.float32))
    got = _run_composite(d, rec, col, 1, counts, offsets, np.zeros(0, np.uint32), w, h, g, g[..., 0], np.ones(n, np.float32), 1, *pre)
    for a, b in zip(got, pre):
        assert np.array_equal(a, b)


def _project_bwd(d, u, planes, strides, n, grec, pre, gdep=None):
    """planes: three buffers (position, scale, rotation) or one interleaved {pos, scale, rot} buffer; gdep: the depth variant."""
    bufs = [d.createBufferFrom(_f(p)) for p in planes] + [d.createBufferFrom(_f(grec))]
    outs = [d.createBufferFrom(_f(pre)) for _ in range(3)]
    offs = [0, 0, 0] if len(planes) == 3 else [0, 16, 32]
    src = bufs[:3] if len(planes) == 3 else [bufs[0]] * 3
    args = (d.ctx, _f(u).ctypes.data_as(C.POINTER(C.c_float)), src[0].ptr + offs[0], strides[0], src[1].ptr + offs[1], strides[1],
            src[2].ptr + offs[2], strides[2], n, bufs[-1].ptr, outs[0].ptr, outs[1].ptr, outs[2].ptr)
    if gdep is None:
        rc = d.lib.splat_project_ellipsoid_backward(*args)
    else:
        gb = d.createBufferFrom(_f(gdep))
        rc = d.lib.splat_project_ellipsoid_backward_depth(*args, gb.ptr)
        bufs.append(gb)
    assert rc == 0
    res = [o.read(np.uint32, n * 4).reshape(n, 4) for o in outs]
    for b in bufs + outs:
        b.destroy()
    return res


@pytest.mark.parametrize("depth", [False, True], ids=["colour", "depth"])
def test_project_backward_strides_are_bit_exact(device, depth):
    w, h = 160, 120
    u = TG.camera_u(w, h)
    for n in (1, 777):
        pos, scl, rot, _ = ER.make_cloud(n, 5, 1.0 if n > 1 else 0.0, 0.03)
        rng = np.random.default_rng(n)
        grec = rng.uniform(-1, 1, (n, 8)).astype(np.float32)
        gdep = rng.uniform(-1, 1, n).astype(np.float32) if depth else None
        pre = np.full((n, 4), SENT.view(np.float32), np.float32)
        ref = _project_bwd(device, u, (pos, scl, rot), (1, 1, 1), n, grec, pre, gdep)
        assert (ref[0][:, 3] == 0).all() and (ref[1][:, 3] == 0).all(), "w word of the position or scale gradient not written as 0"
        assert not (ref[2] == SENT).any()
        assert (ref[0][:, :3] != 0).any()
        # distinct strides per plane (a kernel reading one plane with another's stride fails), then {pos, scale, rot} interleaved
        for ss in ((2, 2, 2), (3, 3, 3), (2, 3, 1), (3, 1, 2), (1, 2, 3)):
            planes = []
            for a, st in zip((pos, scl, rot), ss):
                p = np.full((n * st, 4), np.nan, np.float32)
                p[::st] = a
                planes.append(p)
            got = _project_bwd(device, u, planes, ss, n, grec, pre, gdep)
            assert all(np.array_equal(a, b) for a, b in zip(got, ref)), f"strides {ss}"
        inter = np.stack([pos, scl, rot], 1).reshape(n * 3, 4)
        got = _project_bwd(device, u, (inter,), (3, 3, 3), n, grec, pre, gdep)
        assert all(np.array_equal(a, b) for a, b in zip(got, ref)), "interleaved"


@pytest.mark.parametrize("degree", [0, 1, 2])
def test_sh_backward_stride_48_and_null_opacity(device, degree):
    d = device
    n = 515
    rng = np.random.default_rng(degree)
    pos = np.ones((n, 4), np.float32)
    pos[:, :3] = rng.uniform(-1, 1, (n, 3))
    nb = (degree + 1) ** 2
    sh = rng.normal(0, 0.4, (n, nb * 3)).astype(np.float32)
    gcol = rng.uniform(-1, 1, (n, 4)).astype(np.float32)
    eye = np.array([0.3, -0.2, 4.0], np.float32)

    def run(stride, pos_stride, opacity):
        shb = np.full((n, stride), np.nan, np.float32)
        shb[:, :3 * nb] = sh
        pb = np.full((n * pos_stride, 4), np.nan, np.float32)
        pb[::pos_stride] = pos
        gsh0 = np.zeros((n, stride), np.float32)
        gsh0.view(np.uint32)[:, 3 * nb:] = SENT
        bufs = [d.createBufferFrom(a) for a in (pb, shb, gcol, gsh0, np.full((n, 4), 7.0, np.float32), np.full(n, 7.0, np.float32),
                                                np.ones(n, np.float32))]
        rc = d.lib.splat_sh_colors_backward(d.ctx, eye.ctypes.data_as(C.POINTER(C.c_float)), bufs[0].ptr, pos_stride, bufs[1].ptr,
                                            stride, degree, bufs[6].ptr if opacity else None, bufs[2].ptr, n, bufs[3].ptr, bufs[4].ptr,
                                            bufs[5].ptr)
        assert rc == 0
        out = (bufs[3].read(np.uint32, n * stride).reshape(n, stride), bufs[4].read(np.uint32, n * 4).reshape(n, 4),
               bufs[5].read(np.uint32, n))
        for b in bufs:
            b.destroy()
        return out

    ref = run(3 * nb, 1, True)
    assert (ref[1][:, 3] == 0).all()
    for stride, ps in ((48, 1), (3 * nb + 1, 2), (48, 3)):
        got = run(stride, ps, False)
        assert np.array_equal(got[0][:, :3 * nb], ref[0]), f"sh stride {stride}"
        assert (got[0][:, 3 * nb:] == SENT).all(), f"pad floats written at stride {stride}"
        assert np.array_equal(got[1], ref[1]) and np.array_equal(got[2], ref[2])
