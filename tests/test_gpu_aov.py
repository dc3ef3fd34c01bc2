"""The auxiliary outputs of Gaussian frames (splat_aov: alpha, depth, splat id) on the GPU, against the NumPy restatement of
the contract (tests/aov_ref.py) on the oracle's records and lists.

Staged composites (splat_composite_aov on the oracle's lists): k_composite_px (the default on these screens is forced) or
k_composite (compositeOptions('quadrant')) at tile 16, k_composite_tile at 8, 24 and 32; isotropic PROJECTED, COMPACT, LIT32
records, or disc records (32-byte: alpha and id; DISC48: all three); early-out on and off; colours lit by the kernel or
pre-lit.  Whole frames (Renderer): both frame orders, a screen wider than 256 tiles, a strict band of tile rows, a disc frame,
a C1-size frame; the frame rendered again after an overflow; ComputeShaderRenderer's readers; the JS Renderer and
ComputeShaderRenderer (napi/aov_frame.js) against the Python host bit for bit.  The whole frames run under both composites:
k_composite_px (forced: these screens are below its default threshold) and k_composite.
Every case: rgba8 and rgba32f bit-identical to the same call without the buffers; aov_ref.check's tolerances."""
import ctypes as C
import os
import shutil

import numpy as np
import pytest

import splat_renderer_amd as sr
from oracle import oracle as O
from splat_renderer_amd import _lib
from tests import aov_ref
from tests.helpers import make_case, oracle_pipeline
from tests.test_gpu_stages import TOL_EARLY_OUT_BOUND

pytestmark = pytest.mark.gpu

# (the disc's discard is a step of exp(-3.125) = 0.044 in alpha on rim pixels: those are excluded as near)
FIXTURES = ["tiny7", "small300", "ragged1000"]
KERNELS = [("px", 16), ("quadrant", 16), ("tile", 8), ("tile", 24), ("tile", 32)]
RECORDS = ["projected", "lit32", "compact", "disc", "disc48"]


def load_fixture(name):
    g = np.load(os.path.join(os.path.dirname(__file__), "golden", name + ".npz"))
    w, h = int(g["dims"][1]), int(g["dims"][2])
    return g["props"].astype(np.float32), g["normals"].astype(np.float32), g["uniforms"].astype(np.float32), w, h


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


class Staged:
    """The oracle's records and lists on the device for one (scene, tile size, footprint)."""

    def __init__(self, device, props, normals, u, w, h, tile, disc):
        self.d, self.w, self.h, self.tile, self.disc = device, w, h, tile, disc
        n = props.shape[0]
        self.props, self.normals = props, normals
        if disc:
            proj, discs = O.project_disc(u, props, normals)
            keys, pay = O.extract_keys(proj)
            _, order = O.sort_pairs(keys, pay)
            counts, offsets, idx = O.bin_sorted(proj, order[:n], w, h, tile)
            self.rec_ref, self.z = discs, proj[:, 4]
        else:
            ref = oracle_pipeline(props, normals, u, w, h, tile)
            proj, counts, offsets, idx = ref["proj"], ref["counts"], ref["offsets"], ref["indices"]
            self.rec_ref, self.z = proj, proj[:, 4]
            self.compact = O.project_compact(u, props)
        self.proj, self.counts, self.offsets, self.idx = proj, counts, offsets, idx
        self.bufs = []
        up = lambda a: self._keep(device.createBufferFrom(np.ascontiguousarray(a)))
        self.b_props, self.b_normals = up(props), up(normals)
        self.b_counts, self.b_offsets = up(counts), up(offsets)
        self.b_idx = up(idx if idx.size else np.zeros(1, np.uint32))
        self.b_lit = self._keep(device.createBuffer(n * 16 + 16))
        _lib.check(device.lib.splat_lit_colors(device.ctx, self.b_props.ptr + 16, 2, self.b_normals.ptr, 1, n, self.b_lit.ptr), device.ctx)
        lit = self.b_lit.read(np.float32, n * 4).reshape(n, 4) if n else np.zeros((0, 4), np.float32)
        if disc:
            self.b_disc = up(discs)
            d48 = np.zeros((n, 12), np.float32)
            d48[:, :8], d48[:, 8] = discs, proj[:, 4]
            self.b_disc48 = up(d48)
        else:
            self.b_proj, self.b_compact = up(proj), up(self.compact)
            self.b_lit32 = up(np.concatenate([self.compact, lit], axis=1))
        self.n = n
        self.out = [self._keep(device.createBuffer(w * h * s)) for s in (4, 16, 4, 4, 4)]

    def _keep(self, b):
        self.bufs.append(b)
        return b

    def run(self, fmt, early_out, prelit, aov=True, depth=True):
        d = self.d
        records = {"projected": _lib.RECORDS_PROJECTED, "compact": _lib.RECORDS_COMPACT, "lit32": _lib.RECORDS_LIT32,
                   "disc": _lib.RECORDS_PROJECTED, "disc48": _lib.RECORDS_DISC48}[fmt]
        rbuf = {"projected": "b_proj", "compact": "b_compact", "lit32": "b_lit32", "disc": "b_disc", "disc48": "b_disc48"}[fmt]
        cfg = _lib.CompositeCfg(sr.MODE_FRONT_TO_BACK, int(early_out), self.tile, 0, 0xFFFFFFFF, records, int(prelit),
                                _lib.FOOTPRINT_DISC if self.disc else _lib.FOOTPRINT_ISOTROPIC)
        col, cs = (self.b_lit.ptr, 1) if prelit else (self.b_props.ptr + 16, 2)
        o8, of, od, oa, oi = self.out
        for b in self.out:
            b.zero()
        a = _lib.Aov(od.ptr if depth else None, oa.ptr, oi.ptr) if aov else None
        rc = d.lib.splat_composite_aov(d.ctx, C.byref(cfg), col, cs, self.b_normals.ptr, 1, getattr(self, rbuf).ptr, self.b_idx.ptr,
                                       self.b_counts.ptr, self.b_offsets.ptr, self.w, self.h, o8.ptr, of.ptr, None,
                                       C.byref(a) if a is not None else None)
        _lib.check(rc, d.ctx)
        w, h = self.w, self.h
        res = dict(img8=o8.read(np.uint32).reshape(h, w).copy(), imgf=of.read(np.float32).reshape(h, w, 4).copy())
        if aov:
            res.update(depth=od.read(np.float32).reshape(h, w).copy(), alpha=oa.read(np.float32).reshape(h, w).copy(),
                       id=oi.read(np.uint32).reshape(h, w).copy())
        return res

    def restate(self, early_out):
        stop = None
        if not self.disc:
            _, _, _, stop, near = O.composite(O.MODE_FRONT_TO_BACK, early_out, self.props[:, 4:], self.normals, self.proj, self.idx,
                                              self.counts, self.offsets, self.w, self.h, tile=self.tile, want_stops=True)
        a = aov_ref.restate(self.rec_ref, self.z, self.idx, self.counts, self.offsets, self.w, self.h, self.tile, early_out, stop=stop,
                            disc=self.disc)
        if stop is not None:
            a["near"] |= near.astype(bool)
        return a

    def destroy(self):
        for b in self.bufs:
            b.destroy()


def force(device, kernel):
    device.compositeOptions({"px": "pixel", "quadrant": "quadrant", "tile": None}[kernel])


@pytest.mark.parametrize("name", FIXTURES)
@pytest.mark.parametrize("kernel,tile", KERNELS)
@pytest.mark.parametrize("fmt", RECORDS)
def test_staged_matrix(device, name, kernel, tile, fmt):
    props, normals, u, w, h = load_fixture(name)
    disc = fmt.startswith("disc")
    st = Staged(device, props, normals, u, w, h, tile, disc)
    try:
        force(device, kernel)
        for early_out in (True, False):
            a = st.restate(early_out)
            for prelit in ((False, True) if fmt != "lit32" else (False,)):
                what = f"{name} {kernel} T={tile} {fmt} eo={early_out} prelit={prelit}"
                plain = st.run(fmt, early_out, prelit, aov=False)
                got = st.run(fmt, early_out, prelit, depth=fmt != "disc")
                assert np.array_equal(got["img8"], plain["img8"]), what
                assert np.array_equal(bits(got["imgf"]), bits(plain["imgf"])), what
                assert np.all(got["imgf"][..., 3] == 1.0), what
                aov_ref.check(got["alpha"], got["depth"], got["id"], a, TOL_EARLY_OUT_BOUND, what, check_depth=fmt != "disc")
    finally:
        device.compositeOptions()
        st.destroy()


def test_black_scene_alpha(device):
    """Black splats: the image is bg (1 - alpha), so alpha == 1 - rgba32f.r / 0.05 to 1e-6 — on the GPU alone."""
    props, normals, u, w, h = load_fixture("ragged1000")
    props = props.copy()
    props[:, 4:7] = 0.0
    for kernel, tile in (("px", 16), ("quadrant", 16), ("tile", 24)):
        st = Staged(device, props, normals, u, w, h, tile, False)
        try:
            force(device, kernel)
            got = st.run("projected", True, False)
            assert (got["alpha"] > 0.5).any()
            assert np.abs(got["alpha"] - (1 - got["imgf"][..., 0] / np.float32(0.05))).max() <= 1e-6, kernel
        finally:
            device.compositeOptions()
            st.destroy()


def test_errors(device):
    props, normals, u, w, h = load_fixture("small300")
    st = Staged(device, props, normals, u, w, h, 16, False)
    d = st.d
    o8, of, od, oa, oi = st.out

    def call(mode, aov, fmt=_lib.RECORDS_PROJECTED, footprint=_lib.FOOTPRINT_ISOTROPIC, rec=None):
        cfg = _lib.CompositeCfg(mode, 1, 16, 0, 0xFFFFFFFF, fmt, 0, footprint)
        return d.lib.splat_composite_aov(d.ctx, C.byref(cfg), st.b_props.ptr + 16, 2, st.b_normals.ptr, 1, (rec or st.b_proj).ptr,
                                         st.b_idx.ptr, st.b_counts.ptr, st.b_offsets.ptr, w, h, o8.ptr, of.ptr, None, C.byref(aov))
    try:
        ok = _lib.Aov(od.ptr, oa.ptr, oi.ptr)
        assert call(sr.MODE_FRONT_TO_BACK, ok) == 0
        assert call(sr.MODE_REFERENCE_LITERAL, ok) == -1
        assert call(sr.MODE_FRONT_TO_BACK, _lib.Aov(None, None, None)) == -1
        assert call(sr.MODE_FRONT_TO_BACK, _lib.Aov(od.ptr + 4, oa.ptr, oi.ptr)) == -1
        assert call(sr.MODE_FRONT_TO_BACK, _lib.Aov(od.ptr, oa.ptr, oi.ptr + 8)) == -1
        # 32-byte disc records carry no depth
        sd = Staged(device, props, normals, u, w, h, 16, True)
        try:
            cfg = _lib.CompositeCfg(sr.MODE_FRONT_TO_BACK, 1, 16, 0, 0xFFFFFFFF, _lib.RECORDS_PROJECTED, 0, _lib.FOOTPRINT_DISC)
            args = (d.ctx, C.byref(cfg), sd.b_props.ptr + 16, 2, sd.b_normals.ptr, 1, sd.b_disc.ptr, sd.b_idx.ptr, sd.b_counts.ptr,
                    sd.b_offsets.ptr, w, h, o8.ptr, of.ptr, None)
            assert d.lib.splat_composite_aov(*args, C.byref(_lib.Aov(od.ptr, None, None))) == -1
            assert d.lib.splat_composite_aov(*args, C.byref(_lib.Aov(None, oa.ptr, oi.ptr))) == 0
        finally:
            sd.destroy()
        d.sync()
    finally:
        st.destroy()


def frame_case(device, n, w, h, seed, rs, order, records="lit", tile=16, rows=(0, 0xFFFFFFFF), early_out=True):
    props, normals, u = make_case(n, w, h, seed=seed, radius_scale=rs)
    r = sr.Renderer(device, None, "rgba8unorm", n, tileSize=tile, earlyOut=early_out, frameOrder=order, records=records)
    pm = sr.SplatPropertyManager(device, n)
    pm.setFromArrays(props)
    nb = device.createBufferFrom(normals)
    return props, normals, u, r, pm, nb


def check_frame(device, props, normals, u, r, pm, nb, w, h, tile=16, rows=(0, 0xFFFFFFFF), early_out=True, what=""):
    src = pm.getPropertyBuffer()
    for _ in range(2):  # the second one is a sync-free frame
        r.render(u, src, nb, None, w, h, tileRows=rows, wantFloat=True)
    plain8, plainf = r.readPixels().copy(), r.readPixelsFloat().copy()
    r.aov.ensure(w, h)
    for b, v in ((r.aov.depth, 0x7FC00001), (r.aov.alpha, 0x7FC00002), (r.aov.ids, 0x7FC00003)):  # sentinels
        b.write(np.full(w * h, v, np.uint32))
    r.render(u, src, nb, None, w, h, tileRows=rows, wantFloat=True, wantAov=True)
    got8, gotf = r.readPixels(), r.readPixelsFloat()
    depth, alpha, ids = r.readDepth(), r.readAlpha(), r.readIds()
    assert np.array_equal(got8, plain8) and np.array_equal(bits(gotf), bits(plainf)), what
    nty = -(-h // tile)
    r0, r1 = rows[0], min(rows[1], nty)
    a = aov_ref.iso_reference(props, normals, u, w, h, tile, early_out, rows=(r0, r1))["aov"]
    band = np.zeros((h, w), bool)
    band[r0 * tile:min(r1 * tile, h)] = True
    assert np.all(bits(depth)[~band] == 0x7FC00001) and np.all(bits(alpha)[~band] == 0x7FC00002), what
    assert np.all(ids[~band] == 0x7FC00003), what
    aov_ref.check(alpha, depth, ids, a, TOL_EARLY_OUT_BOUND, what)
    return a


# the whole frames below are on screens of fewer than 2048 tiles, where the library's choice is k_composite: both kernels run
FRAME_KERNELS = ["pixel", "quadrant"]


@pytest.mark.parametrize("kernel", FRAME_KERNELS)
@pytest.mark.parametrize("order", ["tileFirst", "sortFirst"])
@pytest.mark.parametrize("records", ["lit", "projected"])
def test_whole_frame_orders(device, order, records, kernel):
    n, w, h = 20000, 400, 300
    props, normals, u, r, pm, nb = frame_case(device, n, w, h, 3, 1.5, order, records)
    try:
        device.compositeOptions(kernel)
        check_frame(device, props, normals, u, r, pm, nb, w, h, what=f"{order} {records} {kernel}")
    finally:
        device.compositeOptions()
        for o in (r, pm, nb):
            o.destroy()


@pytest.mark.parametrize("kernel", FRAME_KERNELS)
def test_whole_frame_wide_screen_and_band(device, kernel):
    """A screen of more than 256 tiles a side (lit records fall back), and a strict band of tile rows in both frame orders
    (pixels outside it keep their sentinels)."""
    try:
        device.compositeOptions(kernel)
        n, w, h = 20000, 4200, 64
        props, normals, u, r, pm, nb = frame_case(device, n, w, h, 4, 2.0, None)
        try:
            check_frame(device, props, normals, u, r, pm, nb, w, h, what=f"wide {kernel}")
        finally:
            for o in (r, pm, nb):
                o.destroy()
        for order in ("tileFirst", "sortFirst"):
            n, w, h = 20000, 320, 256
            props, normals, u, r, pm, nb = frame_case(device, n, w, h, 5, 1.5, order)
            try:
                check_frame(device, props, normals, u, r, pm, nb, w, h, rows=(3, 9), what=f"band {order} {kernel}")
            finally:
                for o in (r, pm, nb):
                    o.destroy()
    finally:
        device.compositeOptions()


def test_frame_rendered_again_rewrites_the_buffers(device):
    """A sync-free frame that outgrows its pair limit is rendered again by finish(): the buffers read afterwards are that frame's
    (as test_gpu_stages' overflow test makes one)."""
    if os.environ.get("SPLAT_BIN_SYNC") == "1":
        pytest.skip("SPLAT_BIN_SYNC=1: every frame reads its pair total back before it sizes anything: no frame can overflow")
    n, w, h = 20000, 320, 200
    small, normals, u = make_case(n, w, h, 61, 0.5)
    big = small.copy()
    big[:, 3] *= 6.0  # ~20x the pairs
    sbuf, bbuf, nbuf = device.createBufferFrom(small), device.createBufferFrom(big), device.createBufferFrom(normals)
    r = sr.Renderer(device, None, "rgba8unorm", n)
    try:
        for kernel in FRAME_KERNELS:
            device.compositeOptions(kernel)
            r.previousFrameOverflowed = False
            r.render(u, sbuf, nbuf, None, w, h, wantAov=True)  # sync frame: learns the small pair total
            r.render(u, sbuf, nbuf, None, w, h, wantAov=True)  # sync-free
            r.render(u, bbuf, nbuf, None, w, h, wantAov=True)  # sync-free, overflows its limit
            alpha, depth, ids = r.readAlpha(), r.readDepth(), r.readIds()  # finish(): detects, renders it again
            assert r.previousFrameOverflowed
            a = aov_ref.iso_reference(big, normals, u, w, h)["aov"]
            aov_ref.check(alpha, depth, ids, a, TOL_EARLY_OUT_BOUND, f"rendered again ({kernel})")
            r.render(u, sbuf, nbuf, None, w, h)  # and a frame without the buffers: the readers refuse
            with pytest.raises(sr.SplatError):
                r.readIds()
    finally:
        device.compositeOptions()
        for o in (r, sbuf, bbuf, nbuf):
            o.destroy()


@pytest.mark.parametrize("kernel", FRAME_KERNELS)
@pytest.mark.parametrize("records", ["lit", "projected"])
def test_disc_frame(device, records, kernel):
    """A disc frame: depth from its lit disc records (records='lit') or its ProjectedSplat records; the image is unchanged."""
    device.compositeOptions(kernel)
    n, w, h = 20000, 320, 240
    props, normals, u = make_case(n, w, h, seed=23, radius_scale=1.5)
    pm = sr.SplatPropertyManager(device, n)
    pm.setFromArrays(props)
    nb = device.createBufferFrom(normals)
    r = sr.Renderer(device, None, "rgba8unorm", n, earlyOut=True, footprint="disc", records=records)
    st = Staged(device, props, normals, u, w, h, 16, True)
    try:
        r.render(u, pm.getPropertyBuffer(), nb, None, w, h, wantFloat=True)
        plain = bits(r.readPixelsFloat()).copy()
        r.render(u, pm.getPropertyBuffer(), nb, None, w, h, wantFloat=True, wantAov=True)
        assert np.array_equal(bits(r.readPixelsFloat()), plain)
        a = st.restate(True)
        aov_ref.check(r.readAlpha(), r.readDepth(), r.readIds(), a, TOL_EARLY_OUT_BOUND, f"disc frame {records}")
        if records == "projected":  # no ProjectedSplat records, no lit records: no depth
            r2 = sr.Renderer(device, None, "rgba8unorm", n, footprint="disc", records="projected", writeProjected=False)
            with pytest.raises(sr.SplatError):
                r2.render(u, pm.getPropertyBuffer(), nb, None, w, h, wantAov=True)
            r2.destroy()
    finally:
        device.compositeOptions()
        for o in (r, pm, nb, st):
            o.destroy()


def test_compute_shader_renderer_readers(device):
    props, normals, u, w, h = load_fixture("ragged1000")
    st = Staged(device, props, normals, u, w, h, 16, False)
    cr = sr.ComputeShaderRenderer(device, None)
    try:
        cr.render(u, st.b_props, st.b_idx, st.b_normals, st.b_proj, st.b_counts, st.b_offsets, 16, -(-w // 16), w, h, wantAov=True)
        aov_ref.check(cr.readAlpha(), cr.readDepth(), cr.readIds(), st.restate(True), TOL_EARLY_OUT_BOUND, "ComputeShaderRenderer")
    finally:
        cr.destroy()
        st.destroy()


def test_c1_size_frame(device):
    n, w, h = sr.scene.CONFIGS["C1"]
    props, normals, u, r, pm, nb = frame_case(device, n, w, h, 1234, 1.0, None)
    try:
        check_frame(device, props, normals, u, r, pm, nb, w, h, what="C1")
    finally:
        for o in (r, pm, nb):
            o.destroy()


@pytest.mark.skipif(shutil.which("node") is None or not os.path.exists("/usr/include/node/node_api.h"),
                    reason="node / N-API headers not present")
@pytest.mark.parametrize("kernel", ["pixel", "quadrant"])
def test_js_renderer_equals_python(device, tmp_path, kernel):
    """napi/aov_frame.js: the JS Renderer's frame with wantAov (tile-first, ProjectedSplat records) and ComputeShaderRenderer's
    staged composite on its lists — image and all three buffers bit for bit the Python host's; the readers refuse after a frame
    rendered without the buffers."""
    import json
    import subprocess
    import __graft_entry__ as g
    napi = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "splat_renderer_amd", "napi")
    if not os.path.exists(os.path.join(napi, "splat_napi.node")):
        g.build()
    n, w, h = 6000, 256, 192
    props, normals, _ = make_case(n, w, h, seed=77, radius_scale=1.5)
    props.tofile(tmp_path / "props.f32")
    normals.tofile(tmp_path / "normals.f32")
    r = subprocess.run([shutil.which("node"), "aov_frame.js", str(tmp_path / "props.f32"), str(tmp_path / "normals.f32"), str(n),
                        str(w), str(h), str(tmp_path / "js_"), kernel], cwd=napi, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    info = json.loads(r.stdout.strip().splitlines()[-1])
    assert info["refusedWithoutAov"] is True and info["planesEqual"] is True  # (render_frame_planes_aov: the same bytes)
    u = np.array(info["uniforms"], np.float32)
    js = lambda name, dt, shape: np.fromfile(tmp_path / ("js_" + name), dt).reshape(shape)
    try:
        device.compositeOptions(kernel)
        pm = sr.SplatPropertyManager(device, n)
        pm.setFromArrays(props)
        nb = device.createBufferFrom(normals)
        pr = sr.Renderer(device, None, "rgba8unorm", n, frameOrder="tileFirst", records="projected")
        pr.render(u, pm.getPropertyBuffer(), nb, None, w, h)
        with pytest.raises(sr.SplatError):
            pr.readDepth()
        for _ in range(2):
            pr.render(u, pm.getPropertyBuffer(), nb, None, w, h, wantAov=True)
        assert pr.finish() == info["pairs"]
        assert np.array_equal(js("rgba8", np.uint8, (h, w, 4)), pr.readPixels())
        assert np.array_equal(js("depth", np.uint32, (h, w)), bits(pr.readDepth()))
        assert np.array_equal(js("alpha", np.uint32, (h, w)), bits(pr.readAlpha()))
        assert np.array_equal(js("ids", np.uint32, (h, w)), pr.readIds())
        cr = sr.ComputeShaderRenderer(device, None)
        b = pr.binner
        cr.render(u, pm.getPropertyBuffer(), b.getTileIndicesBuffer(), nb, pr.projector.getProjectedBuffer(), b.getTileCountsBuffer(),
                  b.getTileOffsetsBuffer(), 16, -(-w // 16), w, h, wantAov=True)
        assert np.array_equal(js("staged_depth", np.uint32, (h, w)), bits(cr.readDepth()))
        assert np.array_equal(js("staged_alpha", np.uint32, (h, w)), bits(cr.readAlpha()))
        assert np.array_equal(js("staged_ids", np.uint32, (h, w)), cr.readIds())
        for o in (cr, pr, pm, nb):
            o.destroy()
    finally:
        device.compositeOptions()
