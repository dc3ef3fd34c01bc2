"""Every composite kernel on tests/composite_edge.py's adversarial record sets, against the oracle and the float64 evaluation.

The composite is isolated: the oracle's own tile lists (bin_sorted of the records in depth order), counts and offsets are
written into device buffers and handed to the staged ComputeShaderRenderer, for
  - k_composite (compositeOptions("quadrant")), both blends, early-out on and off;
  - k_composite_px, ahead 1 and 2, each cold, warm (two launches before) and under (a launch over empty lists before),
    nearest-on-top only;
  - the default selection on screens of >= 2048 tiles (families a: k_composite_px nearest-on-top);
  - k_composite_tile at T = 1, 8, 10, 24, 32, 64;
with PROJECTED, COMPACT and LIT32 records (family d's free boxes: PROJECTED only).  Then the binner and the composite
together (GPUTileBinner on the same records and depth order), a tile-row band cut through edge records, and the reference's
own edge fixtures (ref_binsorted_edges*.npz) composited at their tile size.

Assertions: test_gpu_stages.check_image_against_oracle's tolerance as it stands; the per-tile {staged, consumed} counters
against the oracle's stops as test_composite_vs_oracle asserts them; where the oracle's pixel is not finite the kernel's is
not either (same channels) and the rgba8 bytes are equal, where it is finite the kernel's is too; every sampled pixel within
composite_edge.composite_f64's bound of the float64 evaluation.
"""
import os

import numpy as np
import pytest

import splat_renderer_amd as sr
from oracle import oracle as O
from splat_renderer_amd import _lib
from tests import composite_edge as E
from tests.helpers import assert_same
from tests.test_composite_edges_cpu import sample_pixels
from tests.test_gpu_stages import TOL_NO_EARLY_OUT, check_image_against_oracle, tile_max

pytestmark = pytest.mark.gpu

SCENES = E.scenes()
MODES = [sr.MODE_FRONT_TO_BACK, sr.MODE_REFERENCE_LITERAL]
KERNELS16 = ["quadrant", "px1", "px1_warm", "px1_under", "px2", "px2_warm", "px2_under"]
TILES = [1, 8, 10, 24, 32, 64]
FORMATS = {"projected": _lib.RECORDS_PROJECTED, "compact": _lib.RECORDS_COMPACT, "lit32": _lib.RECORDS_LIT32}


def cdiv(a, b):
    return -(-a // b)


class Uploaded:
    """One scene's records in every format, its colours (as the property buffer's second half) and normals, on the device."""

    def __init__(self, device, sc):
        self.sc = sc
        self.rec, self.compact, self.col, self.nrm, self.tag = sc.arrays()
        n = self.rec.shape[0]
        props = np.zeros((n, 8), np.float32)
        props[:, 4:] = self.col
        self.bufs = {"props": device.createBufferFrom(props), "nrm": device.createBufferFrom(self.nrm),
                     "projected": device.createBufferFrom(self.rec)}
        if self.compact is not None:
            self.bufs["compact"] = device.createBufferFrom(self.compact)
            self.bufs["lit32"] = device.createBufferFrom(E.lit32(self.compact, self.col, self.nrm))
        self.formats = [f for f in FORMATS if f in self.bufs]

    def destroy(self):
        for b in self.bufs.values():
            b.destroy()


class Lists:
    def __init__(self, device, rec, w, h, tile):
        self.counts, self.offsets, self.idx = E.lists(rec, w, h, tile)
        self.tile, self.ntx, self.nty = tile, cdiv(w, tile), cdiv(h, tile)
        self.bufs = [device.createBufferFrom(a if a.size else np.zeros(1, np.uint32)) for a in (self.idx, self.counts, self.offsets)]

    def destroy(self):
        for b in self.bufs:
            b.destroy()


_F64 = {}


def f64_reference(sc_name, up, mode, early_out):
    key = (sc_name, mode, early_out)
    if key not in _F64:
        sc = up.sc
        counts, offsets, idx = E.lists(up.rec, sc.w, sc.h, 16)
        px, py = sample_pixels(sc.w, sc.h, np.random.default_rng(11), n=3000)
        want, bound, near = E.composite_f64(mode, early_out, up.rec, up.col, up.nrm, counts, offsets, idx, sc.w, sc.h, 16, px, py)
        _F64[key] = (px, py, want, bound, near)
    return _F64[key]


def set_kernel(device, kernel):
    if kernel == "quadrant":
        device.compositeOptions("quadrant")
    elif kernel.startswith("px"):
        device.compositeOptions("pixel", ahead=1 if kernel.startswith("px1") else 2, predict=True)
    else:
        device.compositeOptions()


def render(device, up, L, fmt, mode, early_out, kernel, rows=None, lists_bufs=None):
    """One staged composite of the scene's lists; returns (float image, rgba8 image, per-tile counters)."""
    sc = up.sc
    idx_b, cnt_b, off_b = lists_bufs or L.bufs
    r = sr.ComputeShaderRenderer(device, None, "rgba8unorm", mode=mode, earlyOut=early_out, recordFormat=FORMATS[fmt])
    r.consumedBuffer = device.createBuffer(L.ntx * L.nty * 16)
    if rows is not None:
        r.tileRows = rows
    try:
        set_kernel(device, kernel)
        device.forgetCompositeHistory()
        go = lambda: r.render(None, up.bufs["props"], idx_b, up.bufs["nrm"], up.bufs[fmt], cnt_b, off_b, L.tile, L.ntx, sc.w, sc.h,
                              wantFloat=True)
        if kernel.endswith("_warm"):  # two launches leave costs and an order behind for the third
            go()
            go()
        elif kernel.endswith("_under"):  # a launch over empty lists leaves cost 0 for every tile
            saved = cnt_b.read(np.uint32).copy()
            cnt_b.write(np.zeros_like(saved))
            go()
            cnt_b.write(saved)
        r.consumedBuffer.zero()
        go()
        out = r.readPixelsFloat().copy(), r.readPixels().copy(), r.consumedBuffer.read(np.uint64).reshape(-1, 2).copy()
    finally:
        device.compositeOptions()
        r.destroy()
    return out


def stop_alternatives(col, nrm, rec, idx, counts, offsets, w, h, tile, mode, stop, near, rows=None):
    """The literal blend with early-out: for every pixel the oracle flags `near` (its alpha passed 0.99 within 2e-5), the
    oracle's image had the pixel stopped one entry earlier, or one or two entries later, than the oracle's own stop s —
    the composite of the first k = s - 1, s + 1, s + 2 entries of its tile's list.  Returns a list of (mask, image)."""
    out = []
    nm = near > 0
    for s_ in np.unique(stop[nm]):
        at = nm & (stop == s_)
        for k in (int(s_) - 1, int(s_) + 1, int(s_) + 2):
            if k < 0:
                continue
            img, img8, _ = O.composite(mode, False, col, nrm, rec, idx, np.minimum(counts, k).astype(np.uint32), offsets, w, h,
                                       tile=tile, rows=rows)
            out.append((at, img, img8))
    return out


def check_image(got, got8, want, want8, near, early_out, what, mode=sr.MODE_FRONT_TO_BACK, alts=None):
    """Non-finite pixels first (same channels, same bytes), then the stated tolerance on the rest.  The literal blend with
    early-out: a pixel at the threshold (`near`) that stops one entry earlier or later than the oracle is NOT bounded by
    check_image_against_oracle's (1 - 0.99) * colour — the next entry replaces the colour by up to its Gaussian (:183-185).
    Such a pixel must instead be the oracle's image with the stop moved (alts: stop_alternatives) within TOL_NO_EARLY_OUT
    and 1 LSB; it is then compared as that image's pixel."""
    if mode == sr.MODE_REFERENCE_LITERAL and early_out and alts:
        want, want8 = want.copy(), want8.copy()
        gf = np.where(np.isfinite(got), got, 0.0)
        for at, img, img8 in alts:
            ok = at & (np.abs(gf - np.where(np.isfinite(img), img, 0.0)).max(axis=2) <= TOL_NO_EARLY_OUT) & \
                (np.abs(got8.astype(int) - img8.astype(int)).max(axis=2) <= 1) & \
                (np.isfinite(got[..., :3]) == np.isfinite(img[..., :3])).all(axis=2)
            want[ok], want8[ok] = img[ok], img8[ok]
    bad_w, bad_g = ~np.isfinite(want[..., :3]), ~np.isfinite(got[..., :3])
    assert np.array_equal(bad_w, bad_g), f"{what}: {int((bad_w != bad_g).sum())} channels finite in one image and not in the other"
    nf = bad_w.any(axis=2)
    assert np.array_equal(got8[nf], want8[nf]), f"{what}: rgba8 of non-finite pixels"
    g, wnt = np.where(np.isfinite(got), got, 0.0), np.where(np.isfinite(want), want, 0.0)
    try:
        check_image_against_oracle(g, got8, wnt, want8, near if early_out else None)
    except AssertionError as e:
        err = np.abs(g - wnt).max(axis=2)
        y, x = np.unravel_index(np.argmax(err), err.shape)
        raise AssertionError(f"{what}: worst pixel ({x}, {y}) got {got[y, x]} want {want[y, x]}: {e}") from None
    assert (got8[..., 3] == 255).all()


def check_f64(got, f64, mode, early_out, onear, what):
    px, py, want, bound, near = f64
    g = got[py, px, :3].astype(np.float64)
    assert np.array_equal(np.isfinite(g), np.isfinite(want)), f"{what}: finite where the float64 evaluation is not, or the reverse"
    err = np.where(np.isfinite(g), np.abs(g - np.where(np.isfinite(want), want, 0.0)), 0.0).max(axis=1)
    tol = np.where((near | (onear[py, px] > 0)) & early_out, E.near_tolerance(bound, mode), bound)
    bad = err > tol
    assert not bad.any(), (f"{what}: {int(bad.sum())} sampled pixels beyond the float64 bound, worst "
                           f"({px[np.argmax(err - tol)]}, {py[np.argmax(err - tol)]}) err {err.max():.3g}")


def check_counters(cons, L, stop, near, kernel, mode, early_out, what, rows=None):
    """test_composite_vs_oracle's counter rules: consumed = the tile's largest per-pixel stop wherever no pixel is near the
    threshold; staged by the kernel's batching."""
    counts64 = L.counts.astype(np.uint64)
    r0, r1 = (0, L.nty) if rows is None else rows
    sel = np.zeros((L.nty, L.ntx), bool)
    sel[r0:r1] = True
    sel = sel.reshape(-1)
    tstop, tnear = tile_max(stop, L.tile).reshape(-1), (tile_max(near, L.tile) > 0).reshape(-1)
    ok = sel & ~tnear
    assert_same(cons[ok, 1], tstop[ok].astype(np.uint64), f"{what}: entries consumed per tile")
    # a tile with a pixel at the threshold: that pixel may stop one entry earlier or later than the oracle's (the literal
    # blend's alternatives allow up to two later: see stop_alternatives)
    nt = sel & tnear
    slack = 2 if mode == sr.MODE_REFERENCE_LITERAL else 1
    d = cons[nt, 1].astype(np.int64) - tstop[nt].astype(np.int64)
    assert np.all((d >= -1) & (d <= slack)), f"{what}: entries consumed on tiles at the threshold: off by {d.min()}..{d.max()}"
    assert not cons[~sel].any(), f"{what}: counters of tiles outside the band"
    if not early_out:
        assert_same(cons[sel, 1], counts64[sel], f"{what}: consumed, early-out off")
    px = L.tile == 16 and mode == sr.MODE_FRONT_TO_BACK and (kernel.startswith("px") or (kernel == "default" and L.ntx * L.nty >= 2048))
    if L.tile != 16:
        assert np.all(cons[sel, 1] <= cons[sel, 0]) and np.all(cons[sel, 0] <= counts64[sel]), f"{what}: consumed <= staged <= count"
    elif px and early_out:
        walked = (cons[:, 1] + np.uint64(31)) // np.uint64(32) * np.uint64(32)
        assert np.all(cons[sel, 0] >= np.minimum(counts64, cons[:, 1])[sel]), f"{what}: staged fewer than consumed"
        assert np.all(cons[sel, 0] <= np.minimum(counts64, walked + np.uint64(128))[sel]), f"{what}: staged beyond the look-ahead"
    elif px:
        assert_same(cons[sel, 0], counts64[sel], f"{what}: staged")
    else:
        want = np.minimum(counts64, (cons[:, 1] + np.uint64(255)) // np.uint64(256) * np.uint64(256))
        assert_same(cons[sel, 0], want[sel], f"{what}: staged")


def oracle_image(up, L, mode, early_out, rows=None):
    sc = up.sc
    return O.composite(mode, early_out, up.col, up.nrm, up.rec, L.idx, L.counts, L.offsets, sc.w, sc.h, tile=L.tile,
                       rows=rows, want_stops=True)


def kernels_for(tile, mode, ntiles):
    if tile != 16:
        return ["default"]
    ks = [k for k in KERNELS16 if mode == sr.MODE_FRONT_TO_BACK or not k.startswith("px")]
    if ntiles >= 2048:
        ks.append("default")
    return ks


@pytest.mark.parametrize("name", sorted(SCENES))
@pytest.mark.parametrize("tile", [16] + TILES)
def test_every_kernel_on_edge_records(device, name, tile):
    """One scene, one tile size: every kernel that composites it, both blends, early-out on and off, every record format
    the scene has; image, non-finite pixels, counters, float64 bound."""
    sc = SCENES[name]
    up = Uploaded(device, sc)
    L = Lists(device, up.rec, sc.w, sc.h, tile)
    try:
        for mode in MODES:
            for early_out in (False, True):
                want, want8, _, stop, near = oracle_image(up, L, mode, early_out)
                f64 = f64_reference(name, up, mode, early_out)
                alts = (stop_alternatives(up.col, up.nrm, up.rec, L.idx, L.counts, L.offsets, sc.w, sc.h, tile, mode, stop, near)
                        if mode == sr.MODE_REFERENCE_LITERAL and early_out else None)
                for kernel in kernels_for(tile, mode, L.ntx * L.nty):
                    for fmt in up.formats:
                        what = f"{name} T={tile} mode={mode} early_out={early_out} {kernel} {fmt}"
                        got, got8, cons = render(device, up, L, fmt, mode, early_out, kernel)
                        check_image(got, got8, want, want8, near, early_out, what, mode, alts)
                        check_counters(cons, L, stop, near, kernel, mode, early_out, what)
                        check_f64(got, f64, mode, early_out, near, what)
    finally:
        L.destroy()
        up.destroy()


@pytest.mark.parametrize("name", sorted(SCENES))
def test_binner_and_composite_on_edge_records(device, name):
    """GPUTileBinner on the scene's records in the oracle's depth order gives the oracle's lists; the composite of what it
    leaves (default kernel, nearest on top, early-out on) is the oracle's image."""
    sc = SCENES[name]
    up = Uploaded(device, sc)
    try:
        for tile in (16, 10):
            binner_and_composite(device, up, sc, name, tile)
    finally:
        up.destroy()


def binner_and_composite(device, up, sc, name, tile):
    L = Lists(device, up.rec, sc.w, sc.h, tile)
    keys, pay = O.extract_keys(up.rec)
    _, order = O.sort_pairs(keys, pay)
    sbuf = device.createBufferFrom(order)
    b = sr.GPUTileBinner(device, tile)
    try:
        b.binSplats(None, up.bufs["projected"], sbuf, up.rec.shape[0], sc.w, sc.h, numSorted=order.shape[0])
        assert_same(b.getTileCountsBuffer().read(np.uint32), L.counts, f"{name} T={tile}: counts")
        assert_same(b.getTileOffsetsBuffer().read(np.uint32), L.offsets, f"{name} T={tile}: offsets")
        assert_same(b.getTileIndicesBuffer().read(np.uint32, L.idx.shape[0]), L.idx, f"{name} T={tile}: lists")
        want, want8, _, stop, near = oracle_image(up, L, sr.MODE_FRONT_TO_BACK, True)
        got, got8, cons = render(device, up, L, "projected", sr.MODE_FRONT_TO_BACK, True, "default",
                                 lists_bufs=(b.getTileIndicesBuffer(), b.getTileCountsBuffer(), b.getTileOffsetsBuffer()))
        check_image(got, got8, want, want8, near, True, f"{name} T={tile} binner + composite")
        check_counters(cons, L, stop, near, "default", sr.MODE_FRONT_TO_BACK, True, f"{name} T={tile} binner + composite")
    finally:
        for o in (b, sbuf, L):
            o.destroy()


@pytest.mark.parametrize("name,tile", [("a", 16), ("a", 24), ("a_wide", 64), ("d", 16)])
def test_band_through_edge_records(device, name, tile):
    """A tile-row band [r0, r1) whose edges cut through edge records: its rows are the whole frame's, bit for bit, and the
    oracle's with rows=(r0 * T, r1 * T); counters only inside the band."""
    sc = SCENES[name]
    up = Uploaded(device, sc)
    L = Lists(device, up.rec, sc.w, sc.h, tile)
    r0, r1 = 1, max(2, L.nty - 2)
    try:
        for mode in MODES:
            for kernel in (["default", "px2"] if mode == sr.MODE_FRONT_TO_BACK and tile == 16 else ["default"]):
                whole, whole8, _ = render(device, up, L, "projected", mode, True, kernel)
                got, got8, cons = render(device, up, L, "projected", mode, True, kernel, rows=(r0, r1))
                y0, y1 = r0 * tile, min(r1 * tile, sc.h)
                what = f"{name} T={tile} mode={mode} {kernel} band [{r0}, {r1})"
                assert_same(got[y0:y1].view(np.uint32), whole[y0:y1].view(np.uint32), what)
                assert_same(got8[y0:y1], whole8[y0:y1], what + " rgba8")
                want, want8, _, stop, near = oracle_image(up, L, mode, True, rows=(y0, y1))
                alts = stop_alternatives(up.col, up.nrm, up.rec, L.idx, L.counts, L.offsets, sc.w, sc.h, tile, mode, stop, near,
                                         rows=(y0, y1)) if mode == sr.MODE_REFERENCE_LITERAL else None
                alts = alts and [(m[y0:y1], i[y0:y1], i8[y0:y1]) for m, i, i8 in alts]
                check_image(got[y0:y1], got8[y0:y1], want[y0:y1], want8[y0:y1], near[y0:y1], True, what, mode, alts)
                check_counters(cons, L, stop, near, kernel, mode, True, what, rows=(r0, r1))
    finally:
        L.destroy()
        up.destroy()


@pytest.mark.parametrize("name", ["edges", "edges_t1", "edges_t10", "edges_t24", "edges_t4096"])
def test_reference_edge_lists_composited(device, name):
    """ref_binsorted_edges*.npz — records one ulp either side of tile edges, NaN / inf and straddling records, binned by the
    reference's own code — composited at the fixture's tile size with the fixture's lists, against the oracle."""
    g = np.load(os.path.join(os.path.dirname(__file__), "golden", f"ref_binsorted_{name}.npz"))
    w, h, tile = (int(x) for x in g["dims"])
    rec = g["projected"]
    n = rec.shape[0]
    rng = np.random.default_rng(5)
    col = np.ones((n, 4), np.float32)
    col[:, :3] = rng.uniform(0.1, 1.0, (n, 3))
    nrm = np.zeros((n, 4), np.float32)
    nrm[:, 2] = 1.0
    props = np.zeros((n, 8), np.float32)
    props[:, 4:] = col
    bufs = [device.createBufferFrom(a) for a in (props, nrm, rec, g["indices"], g["counts"], g["offsets"])]
    ntx, nty = cdiv(w, tile), cdiv(h, tile)
    try:
        for mode in MODES:
            for early_out in (False, True):
                for kernel in (["quadrant", "px2"] if tile == 16 and mode == sr.MODE_FRONT_TO_BACK else ["default"]):
                    want, want8, _, stop, near = O.composite(mode, early_out, col, nrm, rec, g["indices"], g["counts"], g["offsets"],
                                                             w, h, tile=tile, want_stops=True)
                    r = sr.ComputeShaderRenderer(device, None, "rgba8unorm", mode=mode, earlyOut=early_out)
                    r.consumedBuffer = device.createBuffer(ntx * nty * 16)
                    r.consumedBuffer.zero()
                    try:
                        set_kernel(device, kernel)
                        device.forgetCompositeHistory()
                        r.render(None, bufs[0], bufs[3], bufs[1], bufs[2], bufs[4], bufs[5], tile, ntx, w, h, wantFloat=True)
                        got, got8 = r.readPixelsFloat(), r.readPixels()
                        cons = r.consumedBuffer.read(np.uint64).reshape(-1, 2)
                    finally:
                        device.compositeOptions()
                        r.destroy()
                    what = f"{name} mode={mode} early_out={early_out} {kernel}"
                    alts = stop_alternatives(col, nrm, rec, g["indices"], g["counts"], g["offsets"], w, h, tile, mode, stop, near) \
                        if mode == sr.MODE_REFERENCE_LITERAL and early_out else None
                    check_image(got, got8, want, want8, near, early_out, what, mode, alts)

                    class _L:
                        pass
                    L = _L()
                    L.counts, L.tile, L.ntx, L.nty = g["counts"], tile, ntx, nty
                    check_counters(cons, L, stop, near, kernel, mode, early_out, what)
    finally:
        for b in bufs:
            b.destroy()
