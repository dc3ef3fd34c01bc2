"""The cameras the ellipsoid (3D Gaussian) tests run under beside the default orbit: named 22-float uniform blocks (VP column-major,
eye, time, W, H), built with oracle.np_oracle.camera and splat_renderer_amd.autograd.pinhole_uniforms only.

The default orbit (distance 3, azimuth 0.5, elevation 0.5, up = +Y, looking at the origin) is a special matrix: no roll, so
VP's m[4] is exactly 0, and a target at the origin, so m[12] = 0 and m[13] ~ 0.  Every term of the projector and of its backward
that one of those entries multiplies is silent under it.  The set below reaches them:

  orbit_default            today's camera (the control)
  orbit_off_target         a target off the origin, seen from below: a non-zero translation column
  pinhole_rolled_offaxis   rolled, fx != fy, the principal point off the centre: all 12 entries the frame reads non-zero
  pinhole_inside           a camera inside the cloud: most splats behind it or reaching w = 0, footprints wider than the screen
  pinhole_top_down         looking down the Y axis with up = +Z: the pose an up = +Y look-at cannot make
  pinhole_subpixel         far away: every footprint is the 0.3 px dilation, and one tile list holds most of the cloud
  pinhole_at_origin        R = I, t = 0 (COLMAP's first camera): the eye is (-0, -0, -0), half the cloud behind it
  general_vp               the default block with rows 0, 1, 3 perturbed entry by entry: no rigid pose (the kernels take any 4x4)

tests/test_ellipsoid_cameras_cpu.py holds the set to its purpose (what each camera keeps on screen, how much of the frame the
image tests skip under it, that one camera has no zero among the 12 entries)."""
import math

import numpy as np
import torch

from oracle import np_oracle as NO
from splat_renderer_amd import autograd as AG

NAMES = ("orbit_default", "orbit_off_target", "pinhole_rolled_offaxis", "pinhole_inside", "pinhole_top_down", "pinhole_subpixel",
         "pinhole_at_origin", "general_vp")
PINHOLES = tuple(n for n in NAMES if n.startswith("pinhole_"))


def look_at(eye, target, roll=0.0, up=(0.0, 1.0, 0.0)):
    """(R, t) float64 of the OpenCV / COLMAP convention (Xc = R X + t; x right, y down, z forward) for a camera at `eye` looking
    at `target`, turned by `roll` radians about its view axis."""
    eye = np.asarray(eye, np.float64)
    f = np.asarray(target, np.float64) - eye
    f /= np.linalg.norm(f)
    r = np.cross(f, np.asarray(up, np.float64))
    r /= np.linalg.norm(r)
    d = np.cross(f, r)
    c, s = math.cos(roll), math.sin(roll)
    R = np.stack([c * r + s * d, -s * r + c * d, f])
    return R, -R @ eye


def pinhole_params(w, h):
    """name -> (R (3, 3), t (3,), fx, fy, cx, cy) float64 of every pinhole camera of the set."""
    def pose(eye, target, fx, fy, cx, cy, roll=0.0, up=(0.0, 1.0, 0.0)):
        R, t = look_at(eye, target, roll, up)
        return R, t, float(fx), float(fy), float(cx), float(cy)
    return {
        "pinhole_rolled_offaxis": pose((1.5, 0.9, -2.0), (0.1, 0.0, 0.0), 150.0, 185.0, 0.37 * w, 0.61 * h, roll=0.65),
        "pinhole_inside": pose((0.2, 0.1, -0.1), (1.0, 0.3, 0.5), 90.0, 90.0, w / 2, h / 2, roll=-0.3),
        "pinhole_top_down": pose((0.05, 3.0, 0.02), (0.0, 0.0, 0.0), 140.0, 140.0, 0.55 * w, 0.45 * h, up=(0.0, 0.0, 1.0)),
        "pinhole_subpixel": pose((9.0, 14.0, -30.0), (0.0, 0.0, 0.0), 200.0, 200.0, w / 2, h / 2, roll=0.2),
        "pinhole_at_origin": (np.eye(3), np.zeros(3), 80.0, 80.0, w / 2, h / 2),
    }


def orbit(w, h, **kw):
    vp, eye = NO.camera(aspect=w / h, **kw)
    u = np.zeros(22, np.float32)
    u[:16], u[16:19], u[20], u[21] = vp, eye, w, h
    return u


def pinhole(w, h, R, t, fx, fy, cx, cy):
    return AG.pinhole_uniforms(torch.as_tensor(R), torch.as_tensor(t), fx, fy, cx, cy, w, h).numpy().astype(np.float32)


def general_vp(w, h):
    """The default block, every entry of rows 0, 1, 3 scaled by 1 + 0.05 N(0, 1), plus 0.4 on m[4], 0.3 on m[12], -0.2 on m[13].
    (The eye stays the orbit's: the depth and the SH direction read it, the records do not.)"""
    u = orbit(w, h)
    m = u[:16].astype(np.float64).reshape(4, 4)  # m[column][row]
    f = 1.0 + 0.05 * np.random.default_rng(9).normal(size=(4, 4))
    f[:, 2] = 1.0
    m = m * f
    m[1, 0] += 0.4
    m[3, 0] += 0.3
    m[3, 1] -= 0.2
    u[:16] = m.reshape(-1).astype(np.float32)
    return u


def cameras(w, h):
    """name -> (22,) float32 uniform block, in NAMES' order."""
    cams = {"orbit_default": orbit(w, h),
            "orbit_off_target": orbit(w, h, target=(0.3, -0.2, 0.4), distance=2.0, azimuth=2.3, elevation=-0.9, fov=70.0)}
    for name, p in pinhole_params(w, h).items():
        cams[name] = pinhole(w, h, *p)
    cams["general_vp"] = general_vp(w, h)
    return {name: cams[name] for name in NAMES}


def camera(name, w, h):
    return cameras(w, h)[name]
