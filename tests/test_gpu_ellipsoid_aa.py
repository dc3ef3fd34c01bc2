"""GPU tests of the antialiased ellipsoid frames (include/splat.h, "antialiased frames": splat_project_ellipsoid_aa,
splat_render_frame_ellipsoids_aa, splat_project_ellipsoid_backward_aa, splat_sampling_rate_max and the antialiased options of
splat_renderer_amd.autograd, .fit and .host) against tests/ellipsoid_aa_ref.py.

Bit-exact: every forward output against the binary32 restatement and against the classic entry points; the backward with
grad_rho = 0 against the three classic backwards; the whole frame against the classic frame fed the compensated plane.
Bounds: the backward against torch float64 autograd under test_gpu_ellipsoid_grad.test_project_backward's criterion (relative
L2 <= 1e-4 per component over well-conditioned splats) and test_gpu_ellipsoid_camera_grad's (1e-4 on the 12 VP entries and on
the eye); the energy a single splat deposits within 2 % of its integral."""
import ctypes as C
import hashlib
import json
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

import splat_renderer_amd as sr
from tests import cameras as CAMS
from tests import ellipsoid_aa_ref as AR
from tests import ellipsoid_camera_grad_ref as CR
from tests import ellipsoid_grad_ref as GR
from tests import ellipsoid_ref as ER
from tests import test_gpu_ellipsoid_grad as TG

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = TG.CASES[:4]
BOUND = 1e-4
SENT = np.uint32(0x7FC0BEEF)  # a quiet NaN with a payload: no kernel arithmetic produces these bits
rel_l2 = CR.rel_l2


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _f(a):
    return np.ascontiguousarray(a, np.float32)


def _fp(a):
    return a.ctypes.data_as(C.POINTER(C.c_float))


def _strided(a, stride):
    """(n, 4) rows `stride` float4s apart, NaN between them."""
    out = np.full((max(a.shape[0], 1) * stride, 4), np.nan, np.float32)
    out[:a.shape[0] * stride:stride] = a
    return out


def project_aa(d, u, pos, scl, rot, col=None, strides=(1, 1, 1, 1), keys=True, want_rho=True, want_col=True, classic=False):
    """splat_project_ellipsoid_aa (or, classic, splat_project_ellipsoid) -> dict(rc, rec, proj, keys, payload, rho, col)."""
    n = pos.shape[0]
    planes = [d.createBufferFrom(_strided(_f(a), s)) for a, s in zip((pos, scl, rot), strides)]
    cbuf = d.createBufferFrom(_strided(_f(col), strides[3])) if col is not None else None
    padded = -(-max(n, 1) // 4096) * 4096 if keys else 0
    rec, proj = d.createBuffer(max(n, 1) * 32), d.createBuffer(max(n, 1) * 32)
    kb = d.createBufferFrom(np.full(max(padded, 1), 0x12345678, np.uint32))
    pb = d.createBufferFrom(np.full(max(padded, 1), 0x12345678, np.uint32))
    rho = d.createBufferFrom(np.full(max(n, 1) + 1, SENT, np.uint32))
    cout = d.createBufferFrom(np.full((max(n, 1) + 1) * 4, SENT, np.uint32))
    head = (d.ctx, _fp(_f(u)), planes[0].ptr, strides[0], planes[1].ptr, strides[1], planes[2].ptr, strides[2], n, proj.ptr, rec.ptr,
            kb.ptr if keys else None, pb.ptr if keys else None, padded)
    if classic:
        rc = d.lib.splat_project_ellipsoid(*head)
    else:
        rc = d.lib.splat_project_ellipsoid_aa(*head, rho.ptr if want_rho else None, cbuf.ptr if cbuf is not None else None, strides[3],
                                              cout.ptr if want_col else None)
    out = dict(rc=rc)
    if rc == 0:
        out.update(rec=rec.read(np.float32, n * 8).reshape(n, 8), proj=proj.read(np.float32, n * 8).reshape(n, 8),
                   keys=kb.read(np.uint32, max(padded, 1)), payload=pb.read(np.uint32, max(padded, 1)), rho=rho.read(np.float32, max(n, 1) + 1),
                   col=cout.read(np.float32, (max(n, 1) + 1) * 4).reshape(-1, 4))
    for b in planes + [rec, proj, kb, pb, rho, cout] + ([cbuf] if cbuf is not None else []):
        b.destroy()
    return out


def check_forward(d, u, pos, scl, rot, col, strides=(1, 1, 1, 1)):
    n = pos.shape[0]
    rec, proj, keys = ER.project(u, pos, scl, rot)
    rho = AR.rho32(u, pos, scl, rot)
    got = project_aa(d, u, pos, scl, rot, col, strides)
    assert got["rc"] == 0
    classic = project_aa(d, u, pos, scl, rot, None, strides, classic=True)
    assert classic["rc"] == 0
    for name, want in (("rec", rec), ("proj", proj)):
        assert np.array_equal(bits(got[name]), bits(want)), f"{name} differs from the restatement"
        assert np.array_equal(bits(got[name]), bits(classic[name])), f"{name} differs from splat_project_ellipsoid"
    assert np.array_equal(got["keys"][:n], keys) and (got["keys"][n:] == 0xFFFFFFFF).all()
    assert np.array_equal(got["keys"], classic["keys"]) and np.array_equal(got["payload"], classic["payload"])
    assert np.array_equal(got["payload"][:n], np.arange(n, dtype=np.uint32))
    assert np.array_equal(bits(got["rho"][:n]), bits(rho)), "rho differs from the restatement"
    assert (bits(got["rho"][n:]) == SENT).all(), "rho written past n"
    cull = ~(rec != 0).any(axis=1)
    assert (bits(got["rho"][:n][cull]) == 0).all()
    assert np.array_equal(bits(got["col"][:n]), bits(AR.compensated(col, rho))), "compensated colour plane differs"
    assert (bits(got["col"][n:]) == SENT).all(), "colour plane written past n"
    return rho, cull


@pytest.mark.parametrize("n,w,h,seed,spread,scale", CASES)
def test_forward_bit_exact(device, n, w, h, seed, spread, scale):
    pos, scl, rot, col = ER.make_cloud(n, seed, spread, scale)
    u = TG.camera_u(w, h)
    rho, cull = check_forward(device, u, pos, scl, rot, col)
    assert cull[[2, 3, 4, 5]].all() and ((rho == 0) & ~cull).sum() == 2 and (rho <= 1).all()
    # without keys, without rho, without the colour plane: the other outputs are the same bits
    a = project_aa(device, u, pos, scl, rot, col, keys=False, want_rho=False)
    b = project_aa(device, u, pos, scl, rot, None, want_col=False)
    rec, proj, _ = ER.project(u, pos, scl, rot)
    for got in (a, b):
        assert got["rc"] == 0 and np.array_equal(bits(got["rec"]), bits(rec)) and np.array_equal(bits(got["proj"]), bits(proj))
    assert (bits(a["rho"]) == SENT).all() and np.array_equal(bits(a["col"][:n]), bits(AR.compensated(col, rho)))
    assert (bits(b["col"]) == SENT).all() and np.array_equal(bits(b["rho"][:n]), bits(rho))


@pytest.mark.parametrize("n", [0, 1, 257])
def test_forward_small_counts_and_strides(device, n):
    pos, scl, rot, col = ER.make_cloud(max(n, 16), 21, 0.8, 0.05)
    pos, scl, rot, col = pos[8:8 + n], scl[8:8 + n], rot[8:8 + n], col[8:8 + n]  # (past the degenerate rows: one live splat at n = 1)
    u = CAMS.camera("pinhole_rolled_offaxis", 96, 64)
    check_forward(device, u, pos, scl, rot, col)
    check_forward(device, u, pos, scl, rot, col, strides=(2, 2, 2, 2))


def test_forward_rejections(device):
    n = 64
    pos, scl, rot, col = ER.make_cloud(n, 3, 0.5, 0.05)
    u = TG.camera_u(64, 64)
    d = device
    b = [d.createBufferFrom(_f(a)) for a in (pos, scl, rot, col)]
    out = [d.createBuffer(n * 32 + 64) for _ in range(4)]
    up = _fp(_f(u))

    def call(**kw):
        a = dict(pos=b[0].ptr, scl=b[1].ptr, rot=b[2].ptr, proj=out[0].ptr, rec=out[1].ptr, rho=out[2].ptr, col=b[3].ptr, cout=out[3].ptr)
        a.update(kw)
        return d.lib.splat_project_ellipsoid_aa(d.ctx, up, a["pos"], 1, a["scl"], 1, a["rot"], 1, n, a["proj"], a["rec"], None, None, 0,
                                                a["rho"], a["col"], 1, a["cout"])
    assert call() == 0
    assert call(rho=None) == 0 and call(cout=None) == 0 and call(col=None, cout=None) == 0 and call(rho=None, col=None, cout=None) == 0
    assert call(col=None) == -1                                  # color_opacity_out requires color_opacity
    assert call(rho=out[2].ptr + 2) == -1                        # rho_out: 4-byte aligned
    assert call(cout=out[3].ptr + 4) == -1 and call(col=b[3].ptr + 4) == -1
    assert call(proj=None) == -1 and call(rec=None) == -1 and call(scl=None) == -1
    assert d.lib.splat_project_ellipsoid_aa(None, up, b[0].ptr, 1, b[1].ptr, 1, b[2].ptr, 1, n, out[0].ptr, out[1].ptr, None, None, 0, None, None,
                                            1, None) == -1
    for x in b + out:
        x.destroy()


# ---- backward --------------------------------------------------------------------------------------------------------------
def backward_aa(d, u, pos, scl, rot, grec, gz, grho, cam=True, which="aa"):
    """(rc, gpos, gscl, grot, grad_uniforms (32 read, 22 written) or None) of splat_project_ellipsoid_backward_aa, or of a classic
    entry point (which = "plain" | "depth" | "camera")."""
    n = pos.shape[0]
    bufs = [d.createBufferFrom(_f(a)) for a in (pos, scl, rot, grec, gz if gz is not None else np.zeros(1), grho)]
    outs = [d.createBuffer(n * 16) for _ in range(3)]
    gu = d.createBufferFrom(np.full(32, SENT, np.uint32))
    head = (d.ctx, _fp(_f(u)), bufs[0].ptr, 1, bufs[1].ptr, 1, bufs[2].ptr, 1, n, bufs[3].ptr, outs[0].ptr, outs[1].ptr, outs[2].ptr)
    gzp = bufs[4].ptr if gz is not None else None
    if which == "aa":
        rc = d.lib.splat_project_ellipsoid_backward_aa(*head, gzp, gu.ptr if cam else None, bufs[5].ptr)
    elif which == "plain":
        rc = d.lib.splat_project_ellipsoid_backward(*head)
    elif which == "depth":
        rc = d.lib.splat_project_ellipsoid_backward_depth(*head, gzp)
    else:
        rc = d.lib.splat_project_ellipsoid_backward_camera(*head, gzp, gu.ptr)
    res = [o.read(np.float32).reshape(n, 4) for o in outs] if rc == 0 else [None] * 3
    g = gu.read(np.float32, count=32) if rc == 0 else None
    for b in bufs + outs + [gu]:
        b.destroy()
    return (rc, *res, g)


def _backward_case(n, w, h, seed, spread, scale):
    pos, scl, rot, _ = ER.make_cloud(n, seed, spread, scale)
    u = TG.camera_u(w, h)
    rng = np.random.default_rng(seed)
    grec = rng.uniform(-1, 1, (n, 8)).astype(np.float32)
    gz = rng.uniform(-1, 1, n).astype(np.float32)
    grho = rng.uniform(-1, 1, n).astype(np.float32)
    cull = GR.culled(u, pos, scl, rot)
    rho = AR.rho32(u, pos, scl, rot)
    kept = (GR.sigma2_cond(u, pos, scl, rot) <= 1e4) & ~cull & (rho > 0)
    return pos, scl, rot, u, grec, gz, grho, cull, rho, kept


@pytest.mark.parametrize("n,w,h,seed,spread,scale", CASES)
def test_backward_against_float64(device, n, w, h, seed, spread, scale):
    pos, scl, rot, u, grec, gz, grho, cull, rho, kept = _backward_case(n, w, h, seed, spread, scale)
    assert kept.sum() > n // 3
    print(f"n={n}: kept {kept.sum()}, rho = 0 among the unculled: {((rho == 0) & ~cull).sum()}")
    live = ~cull & (rho > 0)  # where rho is differentiated; elsewhere its term is exactly zero
    for depth in (False, True):
        P, S, Q = (torch.tensor(a.astype(np.float64), requires_grad=True) for a in (pos, scl, rot))
        L = (GR.records64(u, P, S, Q, ~cull) * torch.as_tensor(grec.astype(np.float64))).sum()
        L = L + (AR.rho64(u, P, S, Q, live) * torch.as_tensor(grho.astype(np.float64))).sum()
        if depth:
            rows = torch.as_tensor(np.nonzero(~cull)[0], dtype=torch.long)
            L = L + (CR.depth64(torch.as_tensor(np.asarray(u, np.float64)), P[rows]) * torch.as_tensor(gz.astype(np.float64))[rows]).sum()
        L.backward()
        rc, gp, gs, gq, _ = backward_aa(device, u, pos, scl, rot, grec, gz if depth else None, grho, cam=False)
        assert rc == 0 and np.isfinite(gp).all() and np.isfinite(gs).all() and np.isfinite(gq).all()
        assert (gp[cull] == 0).all() and (gs[cull] == 0).all() and (gq[cull] == 0).all()
        for name, got, want in (("position", gp, P.grad.numpy()), ("scale", gs, S.grad.numpy()), ("rotation", gq, Q.grad.numpy())):
            for k in range(3 if name != "rotation" else 4):
                e = rel_l2(got[kept, k], want[kept, k])
                print(f"  {'depth' if depth else 'colour'} {name}[{k}]: relative L2 {e:.3g}")
                assert e <= 1e-4, f"{name}[{k}]: relative L2 {e:.3g}"
            if name != "rotation":
                assert (got[:, 3] == 0).all()
        # a splat whose binary32 rho is 0 gets no rho term: the classic backward's bits, whatever its grad_rho
        zero = (rho == 0) & ~cull
        assert zero.sum() == 2
        _, cp, cs, cq, _ = backward_aa(device, u, pos, scl, rot, grec, gz if depth else None, grho, which="depth" if depth else "plain")
        for a, b in ((gp, cp), (gs, cs), (gq, cq)):
            assert np.array_equal(bits(a[zero]), bits(b[zero]))


@pytest.mark.parametrize("n,w,h,seed,spread,scale", CASES)
def test_backward_camera_against_float64(device, n, w, h, seed, spread, scale):
    pos, scl, rot, u, grec, gz, grho, cull, rho, kept = _backward_case(n, w, h, seed, spread, scale)
    # one sum over every unculled splat: ill-conditioned ones are left out through their upstream, as the classic camera test does
    grec[~kept] = 0
    gz[~kept] = 0
    grho[~kept] = 0
    rng = np.random.default_rng(seed + 100)
    grec[cull] = rng.uniform(-1, 1, (int(cull.sum()), 8)).astype(np.float32)  # culled splats add exact zeros whatever they are given
    gz[cull] = 1.0
    grho[cull] = 1.0
    live = ~cull & (rho > 0)
    for depth in (True, False):
        U = CR.utensor(u)
        P, S, Q = (torch.as_tensor(a.astype(np.float64)) for a in (pos, scl, rot))
        L = (CR.records64(U, P, S, Q, ~cull) * torch.as_tensor(grec.astype(np.float64))).sum()
        L = L + (AR.rho64(U, P, S, Q, live) * torch.as_tensor(grho.astype(np.float64))).sum()
        if depth:
            rows = torch.as_tensor(np.nonzero(~cull)[0], dtype=torch.long)
            L = L + (CR.depth64(U, P[rows]) * torch.as_tensor(gz.astype(np.float64))[rows]).sum()
        L.backward()
        want = U.grad.numpy()
        rc, gp, gs, gq, gu = backward_aa(device, u, pos, scl, rot, grec, gz if depth else None, grho)
        assert rc == 0
        g = gu[:22]
        assert np.isfinite(g).all() and (bits(gu[22:]) == SENT).all()
        assert (bits(g[CR.VP_ROW_2]) == 0).all() and (bits(g[19:22]) == 0).all()
        e_vp = rel_l2(g[CR.VP_ROWS_013], want[CR.VP_ROWS_013])
        print(f"n={n} {'depth' if depth else 'colour'}: VP relative L2 {e_vp:.3g}", end="")
        assert e_vp <= BOUND, f"VP relative L2 {e_vp:.3g}"
        if depth:
            e_eye = rel_l2(g[16:19], want[16:19])
            print(f", eye relative L2 {e_eye:.3g}")
            assert e_eye <= BOUND, f"eye relative L2 {e_eye:.3g}"
        else:
            print()
            assert (bits(g[16:19]) == 0).all()
        # the per-splat outputs do not depend on whether the camera sums run, and two runs give the same camera gradient
        rc2, p2, s2, q2, _ = backward_aa(device, u, pos, scl, rot, grec, gz if depth else None, grho, cam=False)
        assert rc2 == 0 and all(np.array_equal(bits(a), bits(b)) for a, b in ((gp, p2), (gs, s2), (gq, q2)))
        again = backward_aa(device, u, pos, scl, rot, grec, gz if depth else None, grho)
        assert np.array_equal(bits(again[4]), bits(gu))


@pytest.mark.parametrize("n,w,h,seed,spread,scale", CASES)
def test_backward_with_zero_grad_rho_is_the_classic_one(device, n, w, h, seed, spread, scale):
    pos, scl, rot, u, grec, gz, _, cull, rho, kept = _backward_case(n, w, h, seed, spread, scale)
    zeros = np.zeros(n, np.float32)
    for which, depth, cam in (("plain", False, False), ("depth", True, False), ("camera", False, True), ("camera", True, True)):
        want = backward_aa(device, u, pos, scl, rot, grec, gz if depth else None, zeros, which=which)
        got = backward_aa(device, u, pos, scl, rot, grec, gz if depth else None, zeros, cam=cam)
        assert want[0] == 0 and got[0] == 0
        for name, a, b in zip(("gpos", "gscl", "grot"), got[1:4], want[1:4]):
            assert np.array_equal(bits(a), bits(b)), f"{which} depth={depth}: {name} differs"
        if cam:
            assert np.array_equal(bits(got[4]), bits(want[4])), f"{which} depth={depth}: grad_uniforms differs"
            again = backward_aa(device, u, pos, scl, rot, grec, gz if depth else None, zeros, cam=True)
            assert np.array_equal(bits(again[4]), bits(got[4]))
        else:
            assert (bits(got[4]) == SENT).all()  # NULL grad_uniforms: nothing written


def test_backward_rejections_and_no_splats(device):
    d = device
    n = 64
    pos, scl, rot, _ = ER.make_cloud(n, 3, 0.5, 0.05)
    u = TG.camera_u(64, 64)
    b = [d.createBufferFrom(_f(a)) for a in (pos, scl, rot, np.zeros((n, 8), np.float32), np.zeros(n + 4, np.float32))]
    out = [d.createBuffer(n * 16 + 64) for _ in range(4)]
    head = (d.ctx, _fp(_f(u)), b[0].ptr, 1, b[1].ptr, 1, b[2].ptr, 1, n, b[3].ptr, out[0].ptr, out[1].ptr, out[2].ptr)
    assert d.lib.splat_project_ellipsoid_backward_aa(*head, None, None, b[4].ptr) == 0
    assert d.lib.splat_project_ellipsoid_backward_aa(*head, None, None, None) == -1          # grad_rho is required
    assert d.lib.splat_project_ellipsoid_backward_aa(*head, None, None, b[4].ptr + 2) == -1  # ... and 4-byte aligned
    assert d.lib.splat_project_ellipsoid_backward_aa(*head, None, out[3].ptr + 4, b[4].ptr) == -1
    gu = d.createBufferFrom(np.full(32, SENT, np.uint32))
    head0 = head[:8] + (0,) + head[9:]
    assert d.lib.splat_project_ellipsoid_backward_aa(*head0, None, gu.ptr, None) == 0        # n = 0: zeros
    g = gu.read(np.float32, count=32)
    assert (bits(g[:22]) == 0).all() and (bits(g[22:]) == SENT).all()
    for x in b + out + [gu]:
        x.destroy()


# ---- whole frames ------------------------------------------------------------------------------------------------------------
def _frame(device, u, pos, scl, rot, col, w, h, antialiased, order=None, records="lit"):
    n = pos.shape[0]
    cloud = sr.GaussianCloud.fromArrays(device, pos, scl, rot, colors=col)
    r = sr.Renderer(device, None, "rgba8unorm", n, footprint="ellipsoid", antialiased=antialiased, frameOrder=order, records=records)
    r.render(u, cloud, None, None, w, h, wantFloat=True, wantAov=True)
    out = dict(img=r.readPixelsFloat().copy(), img8=r.readPixels().copy(), depth=r.readDepth().copy(), alpha=r.readAlpha().copy(),
               ids=r.readIds().copy())
    r.destroy()
    cloud.destroy()
    return out


@pytest.mark.parametrize("n,w,h,seed,spread,scale", CASES)
def test_frame_is_the_classic_frame_of_the_compensated_plane(device, n, w, h, seed, spread, scale):
    pos, scl, rot, col = ER.make_cloud(n, seed, spread, scale)
    u = TG.camera_u(w, h)
    plane = AR.compensated(col, AR.rho32(u, pos, scl, rot))
    for order, records in (("default", "lit"), ("sortFirst", "projected")):
        want = _frame(device, u, pos, scl, rot, plane, w, h, False, order, records)
        got = _frame(device, u, pos, scl, rot, col, w, h, True, order, records)
        for k in ("img", "depth", "alpha"):
            assert np.array_equal(bits(got[k]), bits(want[k])), f"{order}: {k} differs"
        assert np.array_equal(got["ids"], want["ids"]) and np.array_equal(got["img8"], want["img8"]), order
    classic = _frame(device, u, pos, scl, rot, col, w, h, False)
    assert not np.array_equal(bits(classic["img"]), bits(got["img"]))  # (the mode does something)


def test_frame_direct_call_and_empty_cloud(device):
    """splat_render_frame_ellipsoids_aa itself, with n = 0 (the background) and without the optional outputs."""
    d = device
    w, h = 48, 32
    u = TG.camera_u(w, h)
    pos, scl, rot, col = ER.make_cloud(300, 5, 0.5, 0.05)
    cloud = sr.GaussianCloud.fromArrays(d, pos, scl, rot, colors=col)
    sorter, binner = sr.RadixSorter(d, 300), sr.GPUTileBinner(d, 16)
    cfg = TG.cfg()
    imgs = []
    for fn in (d.lib.splat_render_frame_ellipsoids_aa, d.lib.splat_render_frame_ellipsoids):
        out = d.createBuffer(w * h * 16)
        args = (d.ctx, sorter._s, binner._b, C.byref(cfg), _fp(_f(u)), cloud.positions.ptr, cloud.scales.ptr, cloud.rotations.ptr,
                cloud.colorOpacity.ptr, 0, w, h, None, None, out.ptr, None)
        assert fn(*args) == 0
        imgs.append(out.read(np.float32).reshape(h, w, 4))
        out.destroy()
    assert np.array_equal(bits(imgs[0]), bits(imgs[1])) and np.allclose(imgs[0][..., :3], (0.05, 0.05, 0.1))
    bad = TG.cfg(footprint=sr._lib.FOOTPRINT_DISC)
    out = d.createBuffer(w * h * 16)
    assert d.lib.splat_render_frame_ellipsoids_aa(d.ctx, sorter._s, binner._b, C.byref(bad), _fp(_f(u)), cloud.positions.ptr, cloud.scales.ptr,
                                                  cloud.rotations.ptr, cloud.colorOpacity.ptr, 300, w, h, None, None, out.ptr, None) == -1
    for o in (out, sorter, binner, cloud):
        o.destroy()
    with pytest.raises(sr.SplatError):
        sr.Renderer(d, None, "rgba8unorm", 16, antialiased=True)  # the ellipsoid footprint's mode
    p = sr.SplatProjector(d, 16, footprint="ellipsoid")
    with pytest.raises(sr.SplatError):
        p.getCompensationBuffer()
    p.destroy()


def test_projector_compensation_buffer(device):
    n = 3000
    pos, scl, rot, col = ER.make_cloud(n, 1)
    u = TG.camera_u(160, 120)
    cloud = sr.GaussianCloud.fromArrays(device, pos, scl, rot, colors=col)
    p = sr.SplatProjector(device, n, footprint="ellipsoid", antialiased=True)
    p.project(None, u, None, cloud=cloud)
    rec, proj, _ = ER.project(u, pos, scl, rot)
    assert np.array_equal(bits(p.getCompensationBuffer().read(np.float32, n)), bits(AR.rho32(u, pos, scl, rot)))
    assert np.array_equal(bits(p.getDiscBuffer().read(np.float32, n * 8).reshape(n, 8)), bits(rec))
    assert np.array_equal(bits(p.getProjectedBuffer().read(np.float32, n * 8).reshape(n, 8)), bits(proj))
    p.destroy()
    cloud.destroy()


# ---- energy ------------------------------------------------------------------------------------------------------------------
def test_energy_of_a_minified_splat(device):
    """One isotropic splat of screen variance v px^2 and opacity 0.01 on a 64 x 64 screen: the alpha it deposits over the pixel
    grid, divided by the integral of the undilated Gaussian inside the 3-sigma cut, 0.01 2 pi v (1 - e^-4.5)."""
    from splat_renderer_amd import autograd as AG
    w = h = 64
    f, z, o = 64.0, 4.0, 0.01
    u = AG.pinhole_uniforms(torch.eye(3, dtype=torch.float64), torch.zeros(3, dtype=torch.float64), f, f, w / 2, h / 2, w, h).numpy().astype(np.float32)
    r_aa = sr.Renderer(device, None, "rgba8unorm", 1, footprint="ellipsoid", antialiased=True)
    r_classic = sr.Renderer(device, None, "rgba8unorm", 1, footprint="ellipsoid")

    def ratio(r, v, dx, dy):
        s = np.sqrt(v) * z / f
        pos = np.array([[dx * z / f, dy * z / f, z, 1]], np.float32)
        scl = np.array([[s, s, s, 0]], np.float32)
        rot = np.array([[1, 0, 0, 0]], np.float32)
        col = np.array([[1, 1, 1, o]], np.float32)
        cloud = sr.GaussianCloud.fromArrays(device, pos, scl, rot, colors=col)
        r.render(u, cloud, None, None, w, h, wantAov=True)
        total = float(r.readAlpha().astype(np.float64).sum())
        cloud.destroy()
        return total / (o * 2 * np.pi * v * (1 - np.exp(-4.5)))
    for v in (0.02, 0.1, 0.3, 1.0, 4.0, 20.0):
        for dx, dy in ((0.0, 0.0), (0.5, 0.5), (0.25, 0.7), (0.9, 0.1), (0.37, 0.0)):
            q = ratio(r_aa, v, dx, dy)
            print(f"v={v} offset=({dx}, {dy}): deposited / integral = {q:.4f}")
            assert 0.98 <= q <= 1.02, (v, dx, dy, q)
    q = ratio(r_classic, 0.02, 0.25, 0.7)
    print(f"classic v=0.02: {q:.2f}")
    assert q > 10
    r_aa.destroy()
    r_classic.destroy()


# ---- autograd ----------------------------------------------------------------------------------------------------------------
def _leaf(a):
    return torch.tensor(np.ascontiguousarray(a, np.float32), device="cuda", requires_grad=True)


def test_render_gaussians_antialiased_image(device):
    from splat_renderer_amd import autograd as AG
    for (n, w, h, seed) in ((3000, 160, 120, 1), (20000, 333, 200, 2)):
        pos, scl, rot, col, _ = TG._torch_scene(n, w, h, seed)
        u = TG.camera_u(w, h)
        leaves = [_leaf(a) for a in (pos, scl, rot, col[:, 3], col[:, :3])]
        rgb, alpha, depth = AG.render_gaussians(u, *leaves[:4], colors=leaves[4], width=w, height=h, antialiased=True, return_depth=True)
        rec, rho, depths, aux = AG.project_ellipsoids(u, leaves[0], leaves[1], leaves[2], return_depth=True, antialiased=True)
        assert rho.shape == (n,) and rho.requires_grad
        rho32 = AR.rho32(u, pos, scl, rot)
        assert np.array_equal(bits(rho.detach().cpu().numpy()), bits(rho32))
        plane = torch.as_tensor(AR.compensated(col, rho32), device="cuda")
        rgb2, alpha2, depth2 = AG.rasterize(rec, plane, aux, w, h, depths=depths)
        for a, b in ((rgb, rgb2), (alpha, alpha2), (depth, depth2)):
            assert np.array_equal(bits(a.detach().cpu().numpy()), bits(b.detach().cpu().numpy()))
        want = _frame(device, u, pos, scl, rot, col, w, h, True)
        assert np.array_equal(bits(rgb.detach().cpu().numpy()), bits(want["img"][..., :3]))
        # the default is the classic path: the same tuple shapes as before
        assert len(AG.project_ellipsoids(u, leaves[0], leaves[1], leaves[2])) == 2


def test_render_gaussians_antialiased_gradients(device):
    from splat_renderer_amd import autograd as AG
    n, w, h, seed, degree = 3000, 160, 120, 7, 1
    pos, scl, rot, col, sh = TG._torch_scene(n, w, h, seed, degree=degree)
    u = TG.camera_u(w, h)
    cull = GR.culled(u, pos, scl, rot)
    rho32 = AR.rho32(u, pos, scl, rot)
    good = (GR.sigma2_cond(u, pos, scl, rot) <= 1e4) & ~cull & (rho32 > 0)
    assert good.sum() > n // 3
    rec32, counts, offsets, idx = TG.lists(u, pos, scl, rot, w, h)

    def reference(op):
        """The float64 chain under the opacities op: (dL/d{means, scales, rotations, opacities, sh}, dL/du, the upstream g)."""
        col32 = ER.sh_colors(u[16:19], pos, sh, degree, op, dtype=np.float32).astype(np.float32)
        dec = GR.decisions(rec32, AR.compensated(col32, rho32), idx, counts, offsets, w, h)
        g = GR.upstream(w, h, dec["rim"], dec["near"], seed)
        U = CR.utensor(u)
        P, S, Q, OP, SH = (torch.tensor(a.astype(np.float64), requires_grad=True) for a in (pos, scl, rot, op, sh))
        rec = CR.records64(U, GR._v(P, 4, 1.0), GR._v(S), Q, ~cull)
        c = CR.sh_colors64(U[16:19], P, SH, degree, OP, col32[:, :3] > 0)
        rho = AR.rho64(U, P, S, Q, ~cull & (rho32 > 0))
        rgb, alpha = GR.composite64(rec, torch.cat([c[:, :3], c[:, 3:] * rho[:, None]], dim=1), dec["steps"], w, h)
        gt = torch.as_tensor(g.astype(np.float64).reshape(-1, 4))
        ((rgb * gt[:, :3]).sum() + (alpha * gt[:, 3]).sum()).backward()
        return dict(means=P.grad.numpy(), scales=S.grad.numpy(), rotations=Q.grad.numpy(), opacities=OP.grad.numpy(),
                    sh=SH.grad.numpy()), U.grad.numpy(), g

    def run(op, g, deterministic):
        leaves = dict(means=_leaf(pos), scales=_leaf(scl), rotations=_leaf(rot), opacities=_leaf(op), sh=_leaf(sh))
        ut = torch.tensor(u, device="cuda", requires_grad=True)
        rgb_t, alpha_t = AG.render_gaussians(ut, leaves["means"], leaves["scales"], leaves["rotations"], leaves["opacities"], sh=leaves["sh"],
                                             width=w, height=h, degree=degree, antialiased=True, deterministic=deterministic)
        gd = torch.as_tensor(g, device="cuda")
        ((rgb_t * gd[..., :3]).sum() + (alpha_t * gd[..., 3]).sum()).backward()
        return {k: v.grad.detach().cpu().numpy() for k, v in leaves.items()}, ut.grad.detach().cpu().numpy()

    def check_leaves(got, want, label):
        for name in ("means", "scales", "rotations", "opacities", "sh"):
            assert np.isfinite(got[name]).all(), name
            rows = good if name in ("means", "scales", "rotations") else np.ones(n, bool)
            e = rel_l2(got[name][rows].reshape(-1), want[name][rows].reshape(-1))
            print(f"{label} {name}: relative L2 {e:.3g}")
            assert e <= 1e-4, f"{label} {name}: relative L2 {e:.3g}"
    # the splats' gradients on the scene as it is, every opacity kept (test_render_gaussians_gradients' way: rows masked afterwards)
    op = col[:, 3].copy()
    want, _, g = reference(op)
    check_leaves(run(op, g, False)[0], want, "atomic")
    a, b = run(op, g, True), run(op, g, True)
    for name in a[0]:
        assert np.array_equal(bits(a[0][name]), bits(b[0][name])), f"deterministic: {name} differs between two runs"
    assert np.array_equal(bits(a[1]), bits(b[1]))
    check_leaves(a[0], want, "deterministic")
    # the camera's gradient is one sum over all splats, which a row mask cannot reach: ill-conditioned splats are made transparent
    # on both sides for it (test_render_gaussians_camera_gradient's way)
    op0 = np.where(good | cull, col[:, 3], 0).astype(np.float32)
    _, wu, g0 = reference(op0)
    _, gu = run(op0, g0, False)
    e_vp, e_eye = rel_l2(gu[CR.VP_ROWS_013], wu[CR.VP_ROWS_013]), rel_l2(gu[16:19], wu[16:19])
    print(f"uniforms: VP relative L2 {e_vp:.3g}, eye relative L2 {e_eye:.3g}")
    assert e_vp <= BOUND and e_eye <= BOUND
    assert (gu[CR.VP_ROW_2] == 0).all() and (gu[19:22] == 0).all()


# ---- sampling rate and fit ---------------------------------------------------------------------------------------------------
def test_sampling_rate_max(device):
    d = device
    n, w, h = 20001, 160, 120
    pos, _, _, _ = ER.make_cloud(n, 2, 2.5, 0.02)
    pos[9] = [1e30, 0, 0, 1]
    names = ("orbit_default", "pinhole_rolled_offaxis", "pinhole_inside")
    near, margin = 0.2, 0.15
    want = np.zeros(n, np.float32)
    seen_any = np.zeros(n, bool)
    for stride in (1, 2):
        pb = d.createBufferFrom(_strided(_f(pos), stride))
        rb = d.createBufferFrom(np.concatenate([np.zeros(n, np.float32), np.array([SENT], np.uint32).view(np.float32)]))
        want[:] = 0
        for name in names:
            u = CAMS.camera(name, w, h)
            focal = 0.5 * w * float(np.sqrt((u[[0, 4, 8]].astype(np.float64) ** 2).sum()))
            want, seen = AR.sampling_rate(u, focal, near, margin, pos, want)
            seen_any |= seen
            cw = u[3] * pos[:, 0] + u[7] * pos[:, 1] + u[11] * pos[:, 2] + u[15]
            assert ((cw > 0) & (cw <= near)).any() or name != "pinhole_inside"   # splats in front of the eye, behind `near`
            assert ((cw > near) & ~seen).any() and seen.any(), name               # outside the margin, and inside
            assert d.lib.splat_sampling_rate_max(d.ctx, _fp(_f(u)), focal, near, margin, pb.ptr, stride, n, rb.ptr) == 0
        got = rb.read(np.float32)
        assert np.array_equal(bits(got[:n]), bits(want)) and bits(got[n:])[0] == SENT, f"stride {stride}"
        assert (~seen_any).any() and (got[:n][~seen_any] == 0).all()              # seen by no camera: left at zero
        assert d.lib.splat_sampling_rate_max(d.ctx, _fp(_f(u)), 1.0, near, margin, pb.ptr + 4, stride, n, rb.ptr) == -1
        assert d.lib.splat_sampling_rate_max(d.ctx, _fp(_f(u)), 1.0, near, margin, pb.ptr, stride, n, rb.ptr + 2) == -1
        assert d.lib.splat_sampling_rate_max(d.ctx, _fp(_f(u)), 1.0, near, margin, None, stride, 0, None) == 0
        pb.destroy()
        rb.destroy()


def _fit_scene(n, seed, degree=1):
    pos, scl, rot, col = ER.make_cloud(n, seed, 0.8, 0.05, degenerate=False)
    rng = np.random.default_rng(seed)
    sh = rng.normal(0, 0.4, (n, (degree + 1) ** 2, 3)).astype(np.float32)
    return pos[:, :3].copy(), scl[:, :3].copy(), rot, np.clip(col[:, 3], 0.05, 0.95).astype(np.float32), sh


def test_fit_with_both_filters(device, tmp_path):
    from splat_renderer_amd.fit import GaussianFit
    from splat_renderer_amd.ply import load_gaussian_ply
    n, w, h = 600, 96, 64
    pos, scl, rot, op, sh = _fit_scene(n, 41)
    cams = [CAMS.camera(name, w, h) for name in ("orbit_default", "orbit_off_target")]
    fit = GaussianFit(pos, scl, rot, op, sh, antialiased=True, exact_activations=True, deterministic=True)
    assert fit.filter_3d is None
    f3 = fit.update_filter_3d(cams, w, h)
    rate = np.zeros(n, np.float32)
    for u in cams:
        focal = 0.5 * w * float(np.sqrt((u[[0, 4, 8]].astype(np.float64) ** 2).sum()))
        rate, _ = AR.sampling_rate(u, focal, 0.2, 0.15, fit.means.detach().cpu().numpy(), rate)
    with np.errstate(all="ignore"):
        want_f = np.where(rate > 0, np.float32(np.sqrt(0.2)) / rate, 0).astype(np.float32)
    assert np.allclose(f3.cpu().numpy(), want_f, rtol=1e-6, atol=0) and (want_f > 0).sum() > n // 2
    target = torch.full((h, w, 3), 0.4, device="cuda")
    for step in range(3):
        rgb, alpha = fit.render(cams[step % 2], w, h)
        sr.autograd.photometric_loss(rgb, target).backward()
        assert fit.log_scales.grad is not None and torch.isfinite(fit.log_scales.grad).all()
        fit.step()
    assert all(torch.isfinite(p).all() for p in fit.parameters())
    # the saved cloud is the fused one: a viewer that knows nothing of the 3D filter draws what the fit draws
    path = str(tmp_path / "fused.ply")
    fit.save_ply(path)
    g = load_gaussian_ply(path)
    u = cams[0]
    col = ER.sh_colors(u[16:19].astype(np.float64), g["positions"], g["sh"], fit.degree, g["opacity"]).astype(np.float32)
    for antialiased in (False, True):
        fit.antialiased = antialiased
        with torch.no_grad():
            rgb, _ = fit.render(u, w, h)
        got = rgb.cpu().numpy()
        frame = _frame(device, u, g["positions"], g["scales"], g["rotations"], col, w, h, antialiased)["img"][..., :3]
        diff = np.abs(got.astype(np.float64) - frame).max()
        print(f"antialiased={antialiased}: fit.render against the saved PLY's frame: max abs {diff:.3g}")
        # exact_activations' documented bound: an ulp in a scale or an opacity (the fused values go through log and exp once
        # more) now and then carries one pixel across a splat's 3-sigma cut, a step of up to 0.011 x opacity; the ulps themselves
        # move a pixel by less than 1e-4
        assert diff <= 0.011 + 1e-4
        assert (np.abs(got.astype(np.float64) - frame) > 1e-4).sum() <= 24
    # the filter belongs to its rows
    fit.render(u, w, h)[0].sum().backward()
    fit.step()
    fit.densify_and_prune()
    assert fit.filter_3d is None
    fit.update_filter_3d(cams, w, h)
    fit.relocate()
    assert fit.filter_3d is None
    fit.update_filter_3d(cams, w, h)
    fit.add_new(max_splats=fit.n + 10)
    assert fit.filter_3d is None


def fit_digest():
    """sha256 over the parameters and moments of a 300-splat, 20-step deterministic fit constructed without the antialiasing
    arguments (tests/golden/aa_fit_digest.json holds what the commit before them computed)."""
    from splat_renderer_amd.fit import GaussianFit, PLANES
    n, w, h = 300, 96, 64
    pos, scl, rot, op, sh = _fit_scene(n, 43)
    cams = [CAMS.camera(name, w, h) for name in ("orbit_default", "orbit_off_target")]
    fit = GaussianFit(pos, scl, rot, op, sh, deterministic=True)
    yy, xx = np.mgrid[0:h, 0:w]
    target = torch.as_tensor(np.stack([xx / w, yy / h, 0.5 + 0 * xx], axis=2).astype(np.float32), device="cuda")
    for step in range(20):
        rgb, _ = fit.render(cams[step % 2], w, h)
        sr.autograd.photometric_loss(rgb, target).backward()
        fit.step()
    hsh = hashlib.sha256()
    for name in PLANES:
        for t in (getattr(fit, name), fit.m[name], fit.v[name]):
            hsh.update(np.ascontiguousarray(t.detach().cpu().numpy()).tobytes())
    return hsh.hexdigest()


def test_fit_without_the_new_arguments_is_unchanged(device):
    golden = json.load(open(os.path.join(ROOT, "tests", "golden", "aa_fit_digest.json")))
    got = fit_digest()
    assert got == golden["sha256"], "a fit that uses neither filter no longer computes the bytes it did"


def test_js_antialiased_frame_matches_python(device, tmp_path):
    node = shutil.which("node")
    if not node or not os.path.exists("/usr/include/node/node_api.h"):
        pytest.skip("node / N-API headers not present")
    addon = os.path.join(ROOT, "splat_renderer_amd", "napi", "splat_napi.node")
    if not os.path.exists(addon):  # (build it, then fail if it still is not there: a broken addon must not hide behind a skip)
        import __graft_entry__ as g
        g.build()
    assert os.path.exists(addon), "the N-API addon did not build"
    n, w, h = 3000, 160, 120
    pos, scl, rot, col = ER.make_cloud(n, 9, 1.0, 0.03)
    u = TG.camera_u(w, h)
    for name, a in (("pos", pos), ("scl", scl), ("rot", rot), ("col", col), ("u", u)):
        np.ascontiguousarray(a, np.float32).tofile(tmp_path / f"{name}.f32")
    want = _frame(device, u, pos, scl, rot, col, w, h, True)["img8"]
    out = subprocess.run([node, os.path.join(ROOT, "splat_renderer_amd", "napi", "ellipsoid_aa_frame.js"), str(tmp_path), str(n), str(w), str(h)],
                         capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-3000:]
    got = np.fromfile(tmp_path / "out.u8", np.uint8)
    assert np.array_equal(got, np.ascontiguousarray(want).reshape(-1))
