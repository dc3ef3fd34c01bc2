"""CPU checks for the per-splat contribution statistic (include/splat.h, "Contribution of every splat to a frame"): the NumPy
reference the GPU tests compare against (tests/contribution_ref.py) against a brute-force loop and against the composite's
alpha, the ABI's declaration and export, and the selection rule of GaussianFit.prune_by_importance."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests import contribution_ref as CR
from tests import ellipsoid_grad_ref as GR
from tests import ellipsoid_ref as ER
from tests import test_gpu_ellipsoid_grad as TG

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def small():
    n, w, h = 200, 32, 32
    pos, scl, rot, col = ER.make_cloud(n, 5, 0.5, 0.2)
    rec, counts, offsets, idx = TG.lists(TG.camera_u(w, h), pos, scl, rot, w, h)
    dec = GR.decisions(rec, col, idx, counts, offsets, w, h)
    return dict(n=n, w=w, h=h, rec=rec, col=col, counts=counts, offsets=offsets, idx=idx, dec=dec)


@pytest.mark.parametrize("masked,min_weight", [(False, 0.0), (True, 0.01)])
def test_reference_against_brute_force(small, masked, min_weight):
    s = small
    mask = None
    if masked:
        mask = np.random.default_rng(1).uniform(-0.5, 1.5, (s["h"], s["w"])).astype(np.float32)
        mask[3, 4], mask[10, 20] = np.nan, 0.0
    ref = CR.contribution(s["dec"], s["n"], s["w"], s["h"], mask, min_weight)
    bf = CR.brute_force(s["rec"], s["col"], s["idx"], s["counts"], s["offsets"], s["w"], s["h"], mask, min_weight)
    assert ref["pairs"].sum() > 5000 and int(s["counts"].max()) > 64  # a real walk: lists longer than a chunk
    assert np.array_equal(ref["pairs"], bf["pairs"])
    assert (ref["hits_lo"] <= bf["hits"]).all() and (bf["hits"] <= ref["hits_hi"]).all()
    if min_weight == 0:
        assert np.array_equal(ref["hits_lo"], ref["hits_hi"]) and np.array_equal(ref["hits_lo"], ref["pairs"])
    else:
        assert (ref["hits_hi"] < ref["pairs"]).any()
    assert np.allclose(ref["wmax"], bf["wmax"], rtol=1e-12, atol=0)
    assert np.allclose(ref["wsum"], bf["wsum"], rtol=1e-12, atol=1e-300)


def test_summed_weights_are_the_image_alpha(small):
    """sum_i w_i = 1 - T_L per pixel: over all splats, the summed weights are the summed alpha of the composite."""
    s = small
    ref = CR.contribution(s["dec"], s["n"], s["w"], s["h"])
    img = ER.composite(s["rec"], s["col"], np.zeros(s["n"], np.float32), s["idx"], s["counts"], s["offsets"], s["w"], s["h"])
    want = img["alpha"].astype(np.float64).sum()
    assert want > 100 and abs(ref["wsum"].sum() - want) <= 1e-6 * want


def test_header_declares_the_entry_point():
    text = open(os.path.join(ROOT, "include", "splat.h")).read()
    assert re.search(r"#define SPLAT_ABI_VERSION 3\b", text)
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    m = re.search(r"int splat_composite_contribution\s*\(([^)]*)\)\s*;", code)
    assert m, "splat_composite_contribution is not declared"
    args = [a.strip() for a in m.group(1).split(",")]
    assert len(args) == 16 and args[10].endswith("pixel_weight_f32") and args[11] == "float min_weight"
    assert [a.split("*")[-1].strip() for a in args[13:]] == ["hits_u32", "weight_max_f32", "weight_sum_u64"]
    assert "Contribution of every splat to a frame" in text


def test_library_exports_the_entry_point():
    import __graft_entry__ as g
    from splat_renderer_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        g.build()
    lib = C.CDLL(_lib.LIB_PATH)
    assert hasattr(lib, "splat_composite_contribution")
    assert "splat_composite_contribution" in _lib.SIGNATURES and len(_lib.SIGNATURES["splat_composite_contribution"][1]) == 16
    assert _lib.load().splat_abi_version() == 3


SCORES = np.array([0.5, 0.0, 0.25, 0.5, 0.0, 0.75, 0.25, 0.5, 1e-30, 0.0, 0.25], np.float32)


@pytest.mark.parametrize("kw", [dict(keep=1), dict(keep=4), dict(keep=5), dict(keep=0), dict(keep=11), dict(keep=50), dict(keep=0.5),
                                dict(keep=0.05), dict(keep=1.0), dict(threshold=0.25), dict(threshold=0.01), dict(threshold=2.0),
                                dict(threshold=float(np.nextafter(0, 1)))])
def test_selection_rule(kw):
    import torch
    from splat_renderer_amd.fit import select_by_importance
    got = select_by_importance(torch.from_numpy(SCORES), **kw).numpy()
    want = CR.select(SCORES, **kw)
    assert np.array_equal(got, want)
    assert (np.diff(got) > 0).all()
    if "keep" in kw:
        n = SCORES.shape[0]
        k = kw["keep"]
        assert got.shape[0] == (min(n, k) if isinstance(k, int) else max(1, int(k * n)))


def test_selection_rule_ties_and_random():
    import torch
    from splat_renderer_amd.fit import select_by_importance
    # keep=4 of {0.75, 0.5 x3, ...}: the 0.5s at indices 0, 3, 7 all fit; keep=3 drops the last of them, keep=2 the last two
    assert select_by_importance(torch.from_numpy(SCORES), keep=3).tolist() == [0, 3, 5]
    assert select_by_importance(torch.from_numpy(SCORES), keep=2).tolist() == [0, 5]
    assert select_by_importance(torch.from_numpy(SCORES), threshold=float(np.nextafter(0, 1))).tolist() == [0, 2, 3, 5, 6, 7, 8, 10]
    rng = np.random.default_rng(0)
    score = rng.integers(0, 20, 1000).astype(np.float32) / 20  # many ties
    for keep in (100, 0.5, 0.333, 999):
        assert np.array_equal(select_by_importance(torch.from_numpy(score), keep=keep).numpy(), CR.select(score, keep=keep))


def test_selection_rule_rejects_bad_arguments():
    import torch
    from splat_renderer_amd import SplatError
    from splat_renderer_amd.fit import select_by_importance
    s = torch.from_numpy(SCORES)
    for kw in (dict(), dict(threshold=0.1, keep=3), dict(keep=0.0), dict(keep=1.5), dict(keep=-1), dict(keep="half")):
        with pytest.raises(SplatError):
            select_by_importance(s, **kw)
