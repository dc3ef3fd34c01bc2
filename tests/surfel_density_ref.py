"""The surfel entry points of include/splat.h's "Density control and optimiser" block as NumPy, written from the rules and not
from the kernels (tests/density_ref.py's twin): the visibility of a surfel record, one frame's statistics, the plan on a two-column
log-scale plane, and 2DGS's in-plane split.  float64, except where the contract is stated in binary32: the visibility mask and the
screen radius come from oracle.np_oracle.disc_bounds, which restates csrc/disc.h bit for bit.
"""
import numpy as np

from oracle import np_oracle as NO
from tests import density_ref as DR

F = np.float32


def visible(rec, width, height):
    """(mask (n,) bool, radius (n,) float32): disc_bounds succeeds and the box overlaps [0, W) x [0, H); radius = half the box's
    larger side, in binary32: the bits of ProjectedSplat.screenRadius (0 where disc_bounds fails)."""
    bnd, ok = NO.disc_bounds(np.asarray(rec, F))
    with np.errstate(all="ignore"):
        on = ok & (bnd[:, 2] > 0) & (bnd[:, 0] < F(width)) & (bnd[:, 3] > 0) & (bnd[:, 1] < F(height))
        radius = F(0.5) * np.fmax(bnd[:, 2] - bnd[:, 0], bnd[:, 3] - bnd[:, 1])
    return on, radius.astype(F)


def accumulate(rec, grec, width, height, grad_accum, denom, max_radius):
    """One frame: returns (mask uint8, grad_accum, denom, max_radius), the three as new float64 arrays."""
    on, radius = visible(rec, width, height)
    g = np.asarray(grec, np.float64)
    ga, dn, mr = (np.array(a, np.float64) for a in (grad_accum, denom, max_radius))
    ga[on] += np.hypot(g[on, 0] * width / 2, g[on, 1] * height / 2)
    dn[on] += 1
    mr[on] = np.maximum(mr[on], radius[on].astype(np.float64))
    return on.astype(np.uint8), ga, dn, mr


def plan(log_scales, *args, **kw):
    """density_ref.plan on the (n, 2) plane: its max runs over whatever columns there are."""
    log_scales = np.asarray(log_scales)
    assert log_scales.ndim == 2 and log_scales.shape[1] == 2
    return DR.plan(log_scales, *args, **kw)


def apply_geometry(rows, means, log_scales, rotations, seed):
    """splat_densify_geometry_surfel in float64: (means_out (k, 3), log_scales_out (k, 2)).  A split's children are
    mu + R[:, 0] sx xi_x + R[:, 1] sy xi_y with the first two normals of the ellipsoid's draw."""
    rows = np.asarray(rows, np.uint32)
    parent, kind = (rows & DR.PARENT_MASK).astype(np.int64), rows >> 30
    mu, ls = np.asarray(means, np.float64)[parent].copy(), np.asarray(log_scales, np.float64)[parent].copy()
    assert ls.shape[1] == 2
    child = kind >= 2
    if child.any():
        p = parent[child]
        xi = DR.split_normals(p, kind[child] - 2, seed)[:, :2]
        R = DR.rotation_matrices(np.asarray(rotations)[p])
        mu[child] += np.einsum("nij,nj->ni", R[:, :, :2], np.exp(ls[child]) * xi)
        ls[child] -= DR.LOG_SHRINK
    return mu, ls
