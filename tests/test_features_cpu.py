"""CPU checks of the references the feature-channel GPU tests compare against (tests/features_ref.py): the closed-form terms
against torch autograd of the float64 forward, the forward against the image's own composite, the depth-distortion identity
W Q - M^2, the share of masked pixels, and the binary32 restatement's own constants (printed for every scene, order and K)."""
import numpy as np
import pytest
import torch

from tests import composite_grad_terms_ref as CT
from tests import ellipsoid_grad_ref as GR
from tests import features_ref as FR


@pytest.mark.parametrize("K", [1, 5])
@pytest.mark.parametrize("name", FR.SCENES)
def test_closed_form_terms_sum_to_autograd(name, K):
    t64 = FR.terms64(name, K)
    want, gcol_rgb = FR.autograd64(name, K)
    assert (gcol_rgb == 0).all()  # the colour columns of col do not enter a feature map
    assert t64["sum"].shape == want.shape == (CT.scene(name)["n"], FR.NREC + K)
    for k, nm in enumerate(FR.names(K)):
        l2 = CT.rel_l2(t64["sum"][:, k], want[:, k])
        assert np.linalg.norm(want[:, k]) > 0
        assert l2 <= 1e-10, f"{name} K={K} {nm}: relative L2 {l2:.3g}"
    assert (t64["m"] >= np.abs(t64["sum"]) * (1 - 1e-12)).all()


@pytest.mark.parametrize("name", FR.SCENES)
def test_features64_of_rgb_is_the_image_without_its_background(name):
    s = CT.scene(name)
    rec, col = torch.tensor(np.asarray(s["rec"], np.float64)), torch.tensor(np.asarray(s["col"], np.float64))
    with torch.no_grad():
        Fm = FR.features64(rec, col, col[:, :3], s["dec"]["steps"], s["w"], s["h"]).numpy()
        rgb, alpha = GR.composite64(rec, col, s["dec"]["steps"], s["w"], s["h"])
    want = rgb.numpy() - (1 - alpha.numpy())[:, None] * np.array(GR.BG)[None, :]
    assert np.abs(Fm - want).max() <= 1e-12
    assert np.abs(Fm).max() > 0.1


def test_depth_distortion_identity_on_veil():
    """features = (1, z, z^2) gives W, M, Q per pixel; sum over ordered pairs j < i of w_i w_j (z_i - z_j)^2 = W Q - M^2."""
    s = CT.scene("veil")
    lay = s["lay"]
    wk = FR._walk64("veil")
    w = wk["Ti"] * wk["alpha"]
    z = np.asarray(s["z"], np.float64)
    z = (z - z.min()) / (z.max() - z.min())  # (normalised to the scene's depth range, as the recipe advises)
    rec, col = torch.tensor(np.asarray(s["rec"], np.float64)), torch.tensor(np.asarray(s["col"], np.float64))
    zt = torch.tensor(z)
    with torch.no_grad():
        Fm = FR.features64(rec, col, torch.stack([torch.ones_like(zt), zt, zt * zt], dim=1), s["dec"]["steps"], s["w"], s["h"]).numpy()
    got = Fm[:, 0] * Fm[:, 2] - Fm[:, 1] ** 2
    want = np.zeros(s["w"] * s["h"])
    for p, (a, k) in enumerate(zip(lay["start"], lay["K"])):
        wi, zi = w[a:a + k], z[lay["spl"][a:a + k]]
        d = zi[:, None] - zi[None, :]
        want[lay["upix"][p]] = (np.tril(wi[:, None] * wi[None, :] * d * d, -1)).sum()
    assert want.max() > 1e-4
    assert np.abs(got - want).max() <= 1e-9 * np.abs(want).max()


@pytest.mark.parametrize("name", FR.SCENES)
def test_masked_share_is_small(name):
    share = FR.masked(name).mean()
    print(f"{name}: rim | near pixels {100 * share:.1f} %")
    assert share <= 0.15


@pytest.mark.parametrize("K", [1, 5])
@pytest.mark.parametrize("order", FR.ORDERS)
@pytest.mark.parametrize("name", FR.SCENES)
def test_restatement_constants(name, order, K):
    ref = FR.restated(name, order, K)
    print(f"{name} {order} K={K}: c_scene = {ref['c_scene'] * 2 ** 24:.1f} x 2^-24, c_fwd = {ref['c_fwd'] * 2 ** 24:.2f} x 2^-24, relative L2 at most "
          f"{ref['l2'].max():.3g}")
    for c in (ref["c_scene"], ref["c_fwd"]):
        assert np.isfinite(c) and c >= FR.FLOOR
    assert np.isfinite(ref["l2"]).all() and (ref["l2"] < 1e-3).all()
    t32 = FR.terms32(name, order, K)
    assert t32["sum"].dtype == np.float32 and t32["F"].dtype == np.float32
    assert (t32["sum"][~CT.scene(name)["reached"]] == 0).all()
