"""The auxiliary outputs (splat_aov) on a CPU-only box: the entry points are declared, exported, bound and wrapped; the NumPy
restatement (tests/aov_ref.py) agrees with the contract on cases whose answer is known."""
import os
import re

import numpy as np

from oracle import oracle as O
from tests import aov_ref
from tests.helpers import make_case, oracle_pipeline

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("splat_composite_aov", "splat_render_frame_aov", "splat_render_frame_planes_aov")


def test_header_declares_the_aov_entry_points_outside_the_test_hooks():
    text = open(os.path.join(ROOT, "include", "splat.h")).read()
    text = re.sub(r"#ifdef SPLAT_TEST_HOOKS.*?#endif", "", re.sub(r"/\*.*?\*/", "", text, flags=re.S), flags=re.S)
    assert re.search(r"typedef struct splat_aov\s*\{\s*void \*depth_f32;\s*void \*alpha_f32;\s*void \*id_u32;\s*\} splat_aov;", text)
    for name in ENTRY_POINTS:
        assert re.search(rf"\b{name}\s*\([^;]*const splat_aov \*aov\)\s*;", text, flags=re.S), name
    assert "#define SPLAT_ABI_VERSION 3" in text


def test_library_binding_and_addon_cover_the_aov_entry_points():
    import ctypes as C

    import __graft_entry__ as g
    from splat_renderer_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        g.build()
    lib = C.CDLL(_lib.LIB_PATH)
    napi = open(os.path.join(ROOT, "splat_renderer_amd", "napi", "splat_napi.c")).read()
    for name in ENTRY_POINTS:
        assert hasattr(lib, name), name
        assert _lib.SIGNATURES[name][1][-1] == C.POINTER(_lib.Aov), name
        assert f"EXPORT({name[len('splat_'):]})" in napi, name
    assert [f for f, _ in _lib.Aov._fields_] == ["depth_f32", "alpha_f32", "id_u32"]


def test_python_renderers_offer_the_readers():
    import inspect

    import splat_renderer_amd as sr
    for cls in (sr.Renderer, sr.ComputeShaderRenderer):
        assert "wantAov" in inspect.signature(cls.render).parameters
        for m in ("readDepth", "readAlpha", "readIds"):
            assert callable(getattr(cls, m))


def one_splat_case():
    w = h = 48
    proj = np.zeros((1, 8), np.float32)
    cx, cy, r = 20.3, 25.7, 6.0
    proj[0, :4] = [cx - 1.5 * r, cy - 1.5 * r, cx + 1.5 * r, cy + 1.5 * r]
    proj[0, 4], proj[0, 5] = 3.25, r
    counts, offsets, idx = O.bin_sorted(proj, np.zeros(1, np.uint32), w, h, 16)
    return proj, counts, offsets, idx, w, h


def test_one_splat():
    proj, counts, offsets, idx, w, h = one_splat_case()
    a = aov_ref.restate(proj, proj[:, 4], idx, counts, offsets, w, h, 16, True)
    g, _ = aov_ref._iso_g(proj[np.zeros(w * h, np.int64)], (np.arange(w * h) % w + 0.5).astype(np.float32)[:, None],
                          (np.arange(w * h) // w + 0.5).astype(np.float32)[:, None])
    g = g.reshape(h, w)
    cov = g > 0
    assert cov.any() and (~cov).any()
    assert np.all(a["depth"][cov] == np.float32(3.25))
    assert np.all(a["id"][cov] == 0) and np.all(a["id"][~cov] == 0xFFFFFFFF)
    assert np.array_equal(a["alpha"], np.where(cov, np.float32(1) - (np.float32(1) - g), 0).astype(np.float32))
    assert np.all(np.isposinf(a["depth"][~cov])) and np.all(a["alpha"][~cov] == 0)


def test_empty_screen():
    w, h = 40, 24
    proj = np.zeros((0, 8), np.float32)
    counts, offsets, idx = O.bin_sorted(proj, np.zeros(0, np.uint32), w, h, 16)
    a = aov_ref.restate(proj, proj[:, 4], idx, counts, offsets, w, h, 16, True)
    assert np.all(a["alpha"] == 0) and np.all(np.isposinf(a["depth"])) and np.all(a["id"] == 0xFFFFFFFF)


def test_black_scene_alpha_is_the_background_weight():
    """Black splats: the oracle's image is bg (1 - alpha), so alpha = 1 - r / 0.05 to 1e-6."""
    w, h = 96, 64
    props, normals, u = make_case(400, w, h, seed=5, radius_scale=4.0)
    props[:, 4:7] = 0.0
    ref = oracle_pipeline(props, normals, u, w, h)
    img, _, _, stop, near = O.composite(O.MODE_FRONT_TO_BACK, True, props[:, 4:], normals, ref["proj"], ref["indices"],
                                        ref["counts"], ref["offsets"], w, h, want_stops=True)
    a = aov_ref.restate(ref["proj"], ref["proj"][:, 4], ref["indices"], ref["counts"], ref["offsets"], w, h, 16, True, stop=stop)
    assert (a["alpha"] > 0.5).any()
    assert np.abs(a["alpha"] - (1 - img[..., 0] / np.float32(0.05))).max() <= 1e-6


def test_restatement_stops_where_the_oracle_does():
    """The restatement's own stop (used for discs) agrees with the oracle's reported stops on an isotropic scene, except on
    the oracle's near pixels."""
    w, h = 128, 96
    props, normals, u = make_case(1500, w, h, seed=9, radius_scale=2.0)
    ref = aov_ref.iso_reference(props, normals, u, w, h)
    own = aov_ref.restate(ref["proj"], ref["proj"][:, 4], ref["indices"], ref["counts"], ref["offsets"], w, h, 16, True)
    a = ref["aov"]
    m = ~a["near"]
    assert np.abs(own["alpha"][m] - a["alpha"][m]).max() <= 2e-6
    assert np.array_equal(own["id"][m & ~a["id_amb"]], a["id"][m & ~a["id_amb"]])
