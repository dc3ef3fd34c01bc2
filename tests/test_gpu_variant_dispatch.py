"""Every reachable cell of the composite's variant dispatch, on one small scene per footprint.

The host code picks one instantiation of k_composite / k_composite_px / k_composite_tile from the footprint, the record
format, the blend, the early-out, the tile size, the kernel option, whether auxiliary outputs are asked for and whether
per-tile counters are.  Two template arguments swapped in that choice draw a wrong image for the cells concerned only, so
this file walks all of them: a 48 x 40 screen (3 x 3 tiles of 16 with partial tiles on both edges, 6 x 5 tiles of 8), 200
seeded splats, the oracle's own records and tile lists handed to splat_composite_aov.

Per cell: the image with auxiliary outputs equals the image without, bit for bit; the image with counters equals the image
without, bit for bit; the image is the footprint's oracle's within the bound of that kernel's own test (imported from it:
test_gpu_composite_edges, test_gpu_disc, test_gpu_ellipsoid).  The oracles: oracle.oracle's composite and composite_disc
(the ones those tests use; np_oracle restates the first and has no disc composite) and tests/ellipsoid_ref.py.  Every
combination the library refuses returns SPLAT_ERR_INVALID.
"""
import ctypes as C

import numpy as np
import pytest

from oracle import oracle as O
from splat_renderer_amd import _lib
from tests import composite_edge as E
from tests import ellipsoid_ref as ER
from tests import test_gpu_composite_edges as ISO
from tests import test_gpu_disc as DISC
from tests import test_gpu_ellipsoid as ELL
from tests.helpers import make_case

pytestmark = pytest.mark.gpu

W, H, N = 48, 40, 200
ERR_INVALID = -1
F2B, LITERAL = _lib.MODE_FRONT_TO_BACK, _lib.MODE_REFERENCE_LITERAL
# (tile size, compositeOptions kernel, ahead): the three 16-pixel kernels and k_composite_tile
KERNELS = [(16, "quadrant", 0), (16, "pixel", 1), (16, "pixel", 2), (8, None, 0)]
FAMILIES = ["isotropic-projected", "isotropic-compact", "isotropic-lit32", "disc-projected", "disc-disc48", "ellipsoid-projected"]


class Family:
    """One footprint and record format: what splat_composite_aov reads, the lists per tile size, the oracle's images."""

    def __init__(self, device, name):
        self.device, self.name = device, name
        self.footprint, fmt = name.split("-")
        self.fmt = {"projected": _lib.RECORDS_PROJECTED, "compact": _lib.RECORDS_COMPACT, "lit32": _lib.RECORDS_LIT32,
                    "disc48": _lib.RECORDS_DISC48}[fmt]
        self.prelit, self.modes = 0, [F2B]
        if self.footprint == "ellipsoid":
            pos, scl, rot, col = ER.make_cloud(N, 3, 0.6, 0.05)
            self.u = ELL.camera_u(W, H)
            rec, self.proj, _ = ER.project(self.u, pos, scl, rot)
            self.scene = (pos, scl, rot, col)
            self.col, self.nrm, self.prelit = col, np.zeros((N, 4), np.float32), 1
        else:
            props, self.nrm, self.u = make_case(N, W, H, 77, 2.0)
            self.col = props[:, 4:].copy()
            if self.footprint == "disc":
                self.proj, rec = O.project_disc(self.u, props, self.nrm)
                if fmt == "disc48":  # {disc record, depth, -, -, -}
                    rec = np.concatenate([rec, self.proj[:, 4:5], np.zeros((N, 3), np.float32)], axis=1)
            else:
                compact = O.project_compact(self.u, props)
                self.proj = O.expand_compact(compact)  # (the records the composite rebuilds from the compact ones)
                rec = {"projected": self.proj, "compact": compact, "lit32": E.lit32(compact, self.col, self.nrm)}[fmt]
                self.modes = [F2B, LITERAL]
        self.rec = np.ascontiguousarray(rec, np.float32)
        # the 32-byte disc and ellipsoid records carry no depth: alpha and ids only
        self.has_depth = not (self.footprint != "isotropic" and fmt == "projected")
        self.lists = {t: E.lists(self.proj, W, H, t) for t in (16, 8)}
        d = device
        self.bufs = {"col": d.createBufferFrom(self.col), "nrm": d.createBufferFrom(self.nrm), "rec": d.createBufferFrom(self.rec),
                     "img": d.createBuffer(W * H * 16), "img8": d.createBuffer(W * H * 4), "cons": d.createBuffer(6 * 5 * 16),
                     "depth": d.createBuffer(W * H * 4), "alpha": d.createBuffer(W * H * 4), "id": d.createBuffer(W * H * 4)}
        for t, (counts, offsets, idx) in self.lists.items():
            for k, a in (("idx", idx), ("cnt", counts), ("off", offsets)):
                self.bufs[f"{k}{t}"] = d.createBufferFrom(a if a.size else np.zeros(1, np.uint32))
        self._oracle = {}

    def destroy(self):
        for b in self.bufs.values():
            b.destroy()

    def cfg(self, mode, early_out, tile, fmt=None, footprint=None):
        fp = {"isotropic": _lib.FOOTPRINT_ISOTROPIC, "disc": _lib.FOOTPRINT_DISC, "ellipsoid": _lib.FOOTPRINT_ELLIPSOID}
        return _lib.CompositeCfg(mode, int(early_out), tile, 0, _lib.U32_MAX, self.fmt if fmt is None else fmt, self.prelit,
                                 fp[self.footprint] if footprint is None else footprint)

    def launch(self, cfg, tile, aov=False, counters=False, entry="splat_composite_aov"):
        """The return code of one composite of this family's records and lists."""
        b, lib = self.bufs, self.device.lib
        a = _lib.Aov(b["depth"].ptr if self.has_depth else None, b["alpha"].ptr, b["id"].ptr)
        args = [self.device.ctx, C.byref(cfg), b["col"].ptr, 1, b["nrm"].ptr, 1, b["rec"].ptr, b[f"idx{tile}"].ptr, b[f"cnt{tile}"].ptr,
                b[f"off{tile}"].ptr, W, H, b["img8"].ptr, b["img"].ptr, b["cons"].ptr if counters else None]
        if entry != "splat_composite":
            args.append(C.byref(a) if aov else None)
        if entry == "splat_composite_aov_depth":
            args += [b["depth"].ptr, 1]
        return getattr(lib, entry)(*args)

    def render(self, mode, early_out, tile, aov, counters):
        b = self.bufs
        for k in ("img", "img8", "cons"):
            b[k].zero()
        self.device.forgetCompositeHistory()
        _lib.check(self.launch(self.cfg(mode, early_out, tile), tile, aov, counters), self.device.ctx)
        return b["img"].read(np.float32).reshape(H, W, 4), b["img8"].read(np.uint8).reshape(H, W, 4)

    def oracle(self, mode, early_out, tile):
        key = (mode, early_out, tile)
        if key not in self._oracle:
            counts, offsets, idx = self.lists[tile]
            if self.footprint == "isotropic":
                want, want8, _, stop, near = O.composite(mode, early_out, self.col, self.nrm, self.proj, idx, counts, offsets, W, H,
                                                         tile=tile, want_stops=True)
                alts = (ISO.stop_alternatives(self.col, self.nrm, self.proj, idx, counts, offsets, W, H, tile, mode, stop, near)
                        if mode == LITERAL and early_out else None)
                self._oracle[key] = (want, want8, near, alts)
            elif self.footprint == "disc":
                img, img8, _, rim = O.composite_disc(early_out, self.col, self.nrm, self.rec[:, :8], idx, counts, offsets, W, H, tile=tile)
                self._oracle[key] = dict(img=img, img8=img8, rim=rim)
            else:
                self._oracle[key] = ER.composite(self.rec, self.col, self.proj[:, 4], idx, counts, offsets, W, H, tile, early_out)
        return self._oracle[key]

    def check(self, got, got8, mode, early_out, tile, what):
        """The bound of the footprint's own test: test_every_kernel_on_edge_records, test_disc_staged_pipeline_vs_oracle,
        test_staged_pipeline."""
        ref = self.oracle(mode, early_out, tile)
        if self.footprint == "isotropic":
            want, want8, near, alts = ref
            ISO.check_image(got, got8, want, want8, near, early_out, what, mode, alts)
        elif self.footprint == "disc":
            d = np.abs(got - ref["img"]).max(axis=2)
            off_rim = ref["rim"] == 0
            if early_out:
                assert d.max() <= DISC.TOL_RIM, what
                assert d[off_rim].max() <= DISC.TOL_EARLY_OUT_BOUND, what
            else:
                DISC.check_image(got, ref)
                assert np.abs(got8.astype(int) - ref["img8"].astype(int)).max(axis=2)[off_rim].max() <= 1, what
            assert (got8[..., 3] == 255).all(), what
        else:
            ELL.check_image(got, ref, what)
            ELL.check_image8(got8, ref, what)


@pytest.fixture(scope="module", params=FAMILIES)
def family(request, device):
    f = Family(device, request.param)
    yield f
    f.destroy()


def test_every_reachable_cell(device, family):
    f = family
    assert all(c.any() for c, _, _ in f.lists.values()), "the scene reaches no tile"
    cells = 0
    try:
        for tile, kernel, ahead in KERNELS:
            device.compositeOptions(kernel, ahead=ahead)
            for mode in f.modes:
                for early_out in (False, True):
                    what = f"{f.name} mode={mode} early_out={early_out} T={tile} {kernel}{ahead}"
                    plain, plain8 = f.render(mode, early_out, tile, aov=False, counters=False)
                    f.check(plain, plain8, mode, early_out, tile, what)
                    cells += 1
                    # (the reference-literal blend has no auxiliary outputs: test_refused_combinations)
                    for aov, counters in [(False, True)] + ([(True, False), (True, True)] if mode == F2B else []):
                        got, got8 = f.render(mode, early_out, tile, aov, counters)
                        w2 = f"{what} aov={aov} counters={counters}"
                        d = got.view(np.uint32) != plain.view(np.uint32)
                        print(f"{w2}: {int(d.sum())} words differ from the plain image, max {np.abs(got - plain).max():.3g}")
                        assert not d.any(), f"{w2}: the float image is not the plain launch's, bit for bit"
                        assert np.array_equal(got8, plain8), f"{w2}: the rgba8 image is not the plain launch's"
                        cells += 1
    finally:
        device.compositeOptions()
    assert cells == len(KERNELS) * 2 * (4 + (2 if len(f.modes) == 2 else 0))


def test_refused_combinations(device):
    """What the library refuses, it refuses with SPLAT_ERR_INVALID on every kernel and tile size."""
    fams = {n: Family(device, n) for n in ("isotropic-projected", "disc-projected", "ellipsoid-projected")}
    iso, disc, ell = fams.values()
    try:
        for tile, kernel, ahead in KERNELS:
            device.compositeOptions(kernel, ahead=ahead)
            for eo in (False, True):
                for counters in (False, True):
                    what = f"T={tile} {kernel}{ahead} early_out={eo} counters={counters}"
                    # auxiliary outputs with the reference-literal blend
                    assert iso.launch(iso.cfg(LITERAL, eo, tile), tile, aov=True, counters=counters) == ERR_INVALID, what
                    for f in (disc, ell):
                        for aov in (False, True):
                            w2 = f"{what} {f.name} aov={aov}"
                            # compact records, and the reference-literal blend, with a footprint that is not isotropic
                            assert f.launch(f.cfg(F2B, eo, tile, fmt=_lib.RECORDS_COMPACT), tile, aov, counters) == ERR_INVALID, w2
                            assert f.launch(f.cfg(LITERAL, eo, tile), tile, aov, counters) == ERR_INVALID, w2
                            # lit disc records through each public entry point
                            for entry in ("splat_composite", "splat_composite_aov", "splat_composite_aov_depth"):
                                assert f.launch(f.cfg(F2B, eo, tile, fmt=_lib.RECORDS_LIT32), tile, aov, counters, entry) == ERR_INVALID, w2
                    # 48-byte disc records with a footprint that is not the disc
                    for f in (iso, ell):
                        for aov in (False, True):
                            assert f.launch(f.cfg(F2B, eo, tile, fmt=_lib.RECORDS_DISC48), tile, aov, counters) == ERR_INVALID, \
                                f"{what} {f.name} aov={aov}"
    finally:
        device.compositeOptions()
        for f in fams.values():
            f.destroy()
